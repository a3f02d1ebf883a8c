"""ctypes binding of libugsm.so (include/ugsm.h) -- the only native entry into the product.

There is no CPU fallback: if the HIP library is missing or no device is present every
compute call raises (UgsmError).  The pure-host geometry calls work without a GPU.

libugsm_dev.so (include/ugsm_dev.h) is the product's sources plus csrc/dev/: kernel_path 1 (one kernel per reference stage), round 1's
LDS-tiled K-cost (march_min_pixels < 0) and the probe entry points.  Tests and tools reach it through load(dev=True) /
Context(dev=True); a Context that asks for kernel_path 1 or march_min_pixels < 0 gets it by itself.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libugsm.so")
DEV_LIB_PATH = os.path.join(_HERE, "libugsm_dev.so")
UGSM_MAX_BATCH = 16

UGSM_OK = 0
UGSM_ERR_BAD_ARG = 1
UGSM_ERR_SIZE_MISMATCH = 2
UGSM_ERR_TOO_SMALL = 3
UGSM_ERR_NO_DEVICE = 4
UGSM_ERR_DEVICE = 5
UGSM_ERR_NOMEM = 6
UGSM_ERR_STATE = 7
UGSM_PENDING = 8   # not an error: not finished yet (ugsm_poll, ugsm_next_done with block = 0)
UGSM_EMPTY = 9     # not an error: nothing outstanding (ugsm_next_done)
UGSM_ERR_PEER = 10  # the fovea shard: another rank failed its part of the step, or none answered within the deadline
UGSM_SHARD_ID_BYTES = 128
UGSM_MAX_LEVELS = 32

# every symbol include/ugsm.h declares (tests check the library exports all of them)
EXPORTS = [
    "ugsm_default_config", "ugsm_abi_version", "ugsm_is_dev_library", "ugsm_status_string", "ugsm_create", "ugsm_destroy",
    "ugsm_last_error", "ugsm_level_dims", "ugsm_level_iterations", "ugsm_level_smooth_passes",
    "ugsm_threshold_schedule", "ugsm_fovea_dims", "ugsm_pixel_iterations", "ugsm_plan_level", "ugsm_match_full", "ugsm_submit_full_host", "ugsm_submit_foveated_host",
    "ugsm_match_foveated", "ugsm_match_foveated_full", "ugsm_submit_full", "ugsm_submit_foveated", "ugsm_submit_full_batch", "ugsm_submit_foveated_batch", "ugsm_submit_full_batch_host", "ugsm_submit_foveated_batch_host",
    "ugsm_submit_foveated_multi", "ugsm_match_foveated_multi", "ugsm_reconstruct_full_multi",
    "ugsm_wait", "ugsm_wait_all",
    "ugsm_submit_pyramids", "ugsm_submit_fovea_coarse", "ugsm_submit_fovea_fine", "ugsm_triangulate", "ugsm_fovea_mapping", "ugsm_triangulate_fovea", "ugsm_reconstruct_full", "ugsm_stage_pyramid",
    "ugsm_stage_iterate", "ugsm_stage_seed", "ugsm_stage_smooth", "ugsm_stage_weighted_difference", "ugsm_last_iterations", "ugsm_get_kernel_stats",
    "ugsm_stage_lr_check", "ugsm_last_lr_marked", "ugsm_slot_stream",
    "ugsm_reset_kernel_stats", "ugsm_set_profile_events", "ugsm_dev_alloc", "ugsm_dev_free", "ugsm_host_alloc", "ugsm_host_free", "ugsm_copy_to_device", "ugsm_copy_to_host",
    # ABI 5: the queue ...
    "ugsm_poll", "ugsm_enqueue_full", "ugsm_enqueue_foveated", "ugsm_enqueue_full_host", "ugsm_enqueue_foveated_host", "ugsm_enqueue_full_managed",
    "ugsm_enqueue_foveated_managed", "ugsm_flush", "ugsm_next_done", "ugsm_queue_depth", "ugsm_queue_plan",
    # ... and RCCL inside the library
    "ugsm_shard_unique_id", "ugsm_shard_init", "ugsm_shard_init_all", "ugsm_shard_rank", "ugsm_shard_count_ranks", "ugsm_submit_fovea_shard", "ugsm_shard_set_timeout",
    "ugsm_shard_gather", "ugsm_shard_finalize", "ugsm_context_device_bytes",
    # row f-1: the coloured point cloud
    "ugsm_default_cloud_params", "ugsm_cloud_points", "ugsm_point_cloud", "ugsm_point_cloud_fovea",
    # ... and the resized cloud
    "ugsm_resized_cloud_points", "ugsm_point_cloud_resized", "ugsm_point_cloud_resized_fovea",
    # ... and the merged cloud of the whole fovea stack
    "ugsm_fovea_level_mapping", "ugsm_fovea_cloud_points", "ugsm_point_cloud_fovea_all",
    # ... and of the stacks of several windows of one pair
    "ugsm_fovea_multi_cloud_points", "ugsm_point_cloud_fovea_multi",
    # the input formats
    "ugsm_input_bytes_per_pixel", "ugsm_input_format_from_encoding", "ugsm_set_input_format", "ugsm_get_input_format",
    # the LR check of the foveated calls
    "ugsm_set_lr_check", "ugsm_get_lr_check", "ugsm_last_lr_marked_levels",
    # the cloud from the queue
    "ugsm_enqueue_full_cloud", "ugsm_enqueue_foveated_cloud", "ugsm_enqueue_full_cloud_managed", "ugsm_enqueue_foveated_cloud_managed", "ugsm_done_cloud",
    # the checked multi-window call
    "ugsm_submit_foveated_multi_checked", "ugsm_match_foveated_multi_checked",
    # the warped right image and the photometric residual of a match
    "ugsm_warp_planes", "ugsm_warp_right", "ugsm_warp_right_fovea", "ugsm_photometric_residual", "ugsm_photometric_residual_fovea",
    # the checked full-mode call
    "ugsm_submit_full_checked", "ugsm_match_full_checked", "ugsm_last_lr_marked_pair",
    # the seeded full-mode call
    "ugsm_submit_full_seeded", "ugsm_match_full_seeded", "ugsm_stage_restrict", "ugsm_seeded_pixel_iterations",
    # the seeded (warm) foveated call
    "ugsm_submit_foveated_warm", "ugsm_submit_foveated_warm_field", "ugsm_match_foveated_warm", "ugsm_stage_warm_stack", "ugsm_fovea_warm_pixel_iterations",
    # the full-mode call in two halves
    "ugsm_submit_full_coarse", "ugsm_submit_full_fine", "ugsm_match_full_coarse", "ugsm_match_full_fine", "ugsm_stage_prolong", "ugsm_coarse_pixel_iterations",
    # checked full-mode pairs through the queue
    "ugsm_submit_full_checked_host", "ugsm_enqueue_full_checked", "ugsm_enqueue_full_checked_managed", "ugsm_enqueue_full_checked_cloud",
    "ugsm_enqueue_full_checked_cloud_managed", "ugsm_done_checked",
    # the depth image (REP 118)
    "ugsm_default_depth_params", "ugsm_depth_image_size", "ugsm_depth_image", "ugsm_depth_image_fovea", "ugsm_match_full_depth",
    "ugsm_depth_image_fovea_full", "ugsm_depth_image_fovea_multi", "ugsm_match_foveated_depth",
    # lens distortion in triangulation, clouds and depth
    "ugsm_set_lens", "ugsm_get_lens", "ugsm_undistort_points",
]
# ... and what include/ugsm_dev.h adds (libugsm_dev.so only)
DEV_EXPORTS = ["ugsm_stage_poly_probe", "ugsm_stage_div3_probe", "ugsm_stage_div_probe", "ugsm_stage_range_words", "ugsm_stage_iterate_rgb8", "ugsm_stage_level0_direct"]


# input formats (ugsm_set_input_format): the byte layout of the images a context reads; a call on an image in format F gives the rgb8 call's
# result on its conversion to rgb8 (tests/encode_np.py)
UGSM_INPUT_RGB8 = 0
UGSM_INPUT_BGR8 = 1
UGSM_INPUT_RGBA8 = 2
UGSM_INPUT_BGRA8 = 3
UGSM_INPUT_MONO8 = 4
# binary32 images, read as they stand: level 0 of the pyramid is the given floats (finite, >= 0; ugsm.h "FLOAT IMAGES")
UGSM_INPUT_RGB32F = 8
UGSM_INPUT_MONO32F = 9
INPUT_BYTES_PER_PIXEL = {UGSM_INPUT_RGB8: 3, UGSM_INPUT_BGR8: 3, UGSM_INPUT_RGBA8: 4, UGSM_INPUT_BGRA8: 4, UGSM_INPUT_MONO8: 1,
                         UGSM_INPUT_RGB32F: 12, UGSM_INPUT_MONO32F: 4}
INPUT_ENCODINGS = {"rgb8": UGSM_INPUT_RGB8, "bgr8": UGSM_INPUT_BGR8, "rgba8": UGSM_INPUT_RGBA8, "bgra8": UGSM_INPUT_BGRA8,
                   "mono8": UGSM_INPUT_MONO8, "32FC3": UGSM_INPUT_RGB32F, "32FC1": UGSM_INPUT_MONO32F}

# which calls apply the LR check (ugsm_set_lr_check); ugsm_create leaves a context at (lr_check_threshold, UGSM_LR_FULL)
UGSM_LR_FULL = 1
UGSM_LR_FOVEATED = 2

UGSM_DEPTH_32F = 0   # REP 118 32FC1: float32, NaN where there is no reading
UGSM_DEPTH_16U = 1   # REP 118 16UC1: uint16 millimetres, 0 where there is no reading
UGSM_DEPTH_ALL_LEVELS = -1
DEPTH_DTYPES = {UGSM_DEPTH_32F: np.dtype(np.float32), UGSM_DEPTH_16U: np.dtype(np.uint16)}
DEPTH_ENCODINGS = {"32FC1": UGSM_DEPTH_32F, "16UC1": UGSM_DEPTH_16U}

UGSM_CLOUD_PCL32 = 0     # pcl::PointXYZRGB in memory: x, y, z, 1.0f, rgb word, 12 zero bytes (32 B)
UGSM_CLOUD_XYZRGB16 = 1  # x, y, z, rgb word (16 B)
# the records as numpy structured dtypes (explicit offsets; rgb is the packed R << 16 | G << 8 | B word)
CLOUD_PCL32 = np.dtype({"names": ["x", "y", "z", "w", "rgb"], "formats": [np.float32, np.float32, np.float32, np.float32, np.uint32],
                        "offsets": [0, 4, 8, 12, 16], "itemsize": 32})
CLOUD_XYZRGB16 = np.dtype({"names": ["x", "y", "z", "rgb"], "formats": [np.float32, np.float32, np.float32, np.uint32],
                           "offsets": [0, 4, 8, 12], "itemsize": 16})
CLOUD_DTYPES = {UGSM_CLOUD_PCL32: CLOUD_PCL32, UGSM_CLOUD_XYZRGB16: CLOUD_XYZRGB16}


class UgsmError(RuntimeError):
    def __init__(self, status: int, what: str, tag=None):
        super().__init__(f"ugsm status {status}: {what}")
        self.status = status
        self.tag = tag   # next_done: the pair whose call failed (the completion HAS been consumed: the caller forgets the tag, then handles the error)


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("levels", C.c_int), ("fovea_levels", C.c_int), ("slots", C.c_int),
                ("kernel_path", C.c_int), ("profile_events", C.c_int), ("march_min_pixels", C.c_int), ("march_np", C.c_int),
                ("march_rows", C.c_int), ("march_smooth", C.c_int), ("early_exit_threshold", C.c_float), ("small_max_pixels", C.c_int),
                ("lr_check_threshold", C.c_float), ("streams", C.c_int), ("batch", C.c_int), ("stream_priority", C.c_int)]


class CloudParams(C.Structure):
    """ugsm_cloud_params (include/ugsm.h)."""
    _fields_ = [("sampling", C.c_int), ("format", C.c_int), ("compact", C.c_int), ("min_conf", C.c_float), ("z_min", C.c_float),
                ("z_max", C.c_float)]


class DepthParams(C.Structure):
    """ugsm_depth_params (include/ugsm.h)."""
    _fields_ = [("format", C.c_int), ("unit", C.c_float), ("min_conf", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float),
                ("factor", C.c_float)]


class QueueCloud(C.Structure):
    """ugsm_queue_cloud (include/ugsm.h): the cloud job a pair is enqueued with."""
    _fields_ = [("P1", C.c_double * 12), ("P2", C.c_double * 12), ("params", CloudParams), ("max_points", C.c_longlong), ("want_planes", C.c_int),
                ("reserved", C.c_int)]


class CloudResult(C.Structure):
    """ugsm_cloud_result (include/ugsm.h): what ugsm_done_cloud reports."""
    _fields_ = [("points", C.c_void_p), ("count", C.c_longlong), ("stored", C.c_longlong), ("point_step", C.c_int), ("levels", C.c_int),
                ("level_counts", C.c_longlong * UGSM_MAX_LEVELS)]


class CheckedResult(C.Structure):
    """ugsm_checked_result (include/ugsm.h): what ugsm_done_checked reports."""
    _fields_ = [("back", C.POINTER(C.c_float) * 3), ("marked_fwd", C.c_longlong), ("marked_back", C.c_longlong)]


def queue_cloud(P1, P2, params: CloudParams, max_points: int = 0, want_planes: bool = False) -> QueueCloud:
    """A ugsm_queue_cloud from two 3x4 projection matrices and the cloud's parameters."""
    q = QueueCloud()
    q.P1[:] = np.ascontiguousarray(P1, np.float64).reshape(12).tolist()
    q.P2[:] = np.ascontiguousarray(P2, np.float64).reshape(12).tolist()
    C.memmove(C.byref(q.params), C.byref(params), C.sizeof(CloudParams))
    q.max_points = int(max_points)
    q.want_planes = 1 if want_planes else 0
    return q


class LevelPlan(C.Structure):
    _fields_ = [("cost_kernel", C.c_int), ("smooth_kernel", C.c_int), ("smooth_rh", C.c_int), ("strip_rows", C.c_int), ("seed_fused", C.c_int),
                ("smooth_tile_rows", C.c_int), ("alone", C.c_int), ("pairs_per_launch", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("level", C.c_int), ("reserved", C.c_int), ("launches", C.c_longlong),
                ("total_ms", C.c_double), ("pixel_launches", C.c_double)]


class Completion(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("status", C.c_int), ("slot", C.c_int), ("call_pairs", C.c_int), ("reserved", C.c_int),
                ("call_index", C.c_longlong), ("done_ns", C.c_longlong), ("result", C.POINTER(C.c_float) * 5)]


_libs = {}


def _elf_dynamic(path: str):
    """(SONAME, [DT_NEEDED ...]) of a 64-bit little-endian ELF shared object, read from its dynamic section; (None, []) if the file is not
    one.  Enough of a reader to compare which HIP runtime ABI two libraries name -- no external tool."""
    import struct
    try:
        with open(path, "rb") as f:
            data = f.read()
        if data[:6] != b"\x7fELF\x02\x01":
            return None, []
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
        dyn = next((sec for sec in secs if sec[1] == 6), None)   # SHT_DYNAMIC
        if dyn is None:
            return None, []
        strtab = secs[dyn[6]]                                     # sh_link: its string table
        def name(off):
            a = strtab[4] + off
            return data[a:data.index(b"\0", a)].decode()
        soname, needed = None, []
        for i in range(dyn[5] // 16):
            tag, val = struct.unpack_from("<qQ", data, dyn[4] + 16 * i)
            if tag == 0:
                break
            if tag == 14:
                soname = name(val)
            elif tag == 1:
                needed.append(name(val))
        return soname, needed
    except (OSError, ValueError, struct.error, IndexError, StopIteration):
        return None, []


def _torch_hip_runtime_path():
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return path if os.path.exists(path) else None


def _share_torch_hip_runtime(lib_path: str = LIB_PATH, torch_hip: str | None = None):
    """PyTorch's ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  A process that loads libugsm.so FIRST (which brings in
    /opt/rocm's runtime) and imports torch afterwards ends up with two HIP runtimes, and the second one finds no GPU ("No HIP GPUs are
    available").  When torch is installed, its runtime is therefore loaded first, globally, and libugsm.so binds to it -- the order
    bench.py and the tools have always used (they import torch first).  A host without torch (the ROS node) is not affected.
    Only when the two name the SAME runtime ABI: libugsm.so was compiled against /opt/rocm's headers and asks for one SONAME
    (DT_NEEDED libamdhip64.so.N); a torch wheel built for another ROCm major carries another, and binding libugsm.so's HIP calls to it
    would be an ABI gamble -- then nothing is preloaded and a warning says so.  UGSM_NO_TORCH_RUNTIME=1 switches the preload off.
    Returns what happened: "preloaded", "off", "no torch", "mismatch" or "failed"."""
    import warnings
    if os.environ.get("UGSM_NO_TORCH_RUNTIME") == "1":
        return "off"
    try:
        path = torch_hip if torch_hip is not None else _torch_hip_runtime_path()
    except Exception as e:  # noqa: BLE001  (a broken torch installation must not keep the library from loading)
        warnings.warn(f"ug_stereomatcher_amd: could not look for PyTorch's HIP runtime ({e}); libugsm.so uses the system's", RuntimeWarning)
        return "failed"
    if path is None:
        return "no torch"
    wanted = next((n for n in _elf_dynamic(lib_path)[1] if n.startswith("libamdhip64.so")), None)
    offered = _elf_dynamic(path)[0]
    if wanted is None or offered != wanted:
        warnings.warn(f"ug_stereomatcher_amd: PyTorch bundles HIP runtime {offered!r} but libugsm.so was built against {wanted!r}: not sharing it -- "
                      "import torch BEFORE this package if both are to see the GPU, or rebuild libugsm.so against torch's ROCm", RuntimeWarning)
        return "mismatch"
    try:
        C.CDLL(path, mode=C.RTLD_GLOBAL)
        return "preloaded"
    except OSError as e:
        warnings.warn(f"ug_stereomatcher_amd: could not preload {path} ({e}); a later `import torch` may not see the GPU", RuntimeWarning)
        return "failed"


def load(dev: bool = False):
    """Loads libugsm.so (dev: libugsm_dev.so); raises if it has not been built (python __graft_entry__.py / make -C csrc)."""
    if dev in _libs:
        return _libs[dev]
    path = DEV_LIB_PATH if dev else LIB_PATH
    if not os.path.exists(path):
        raise UgsmError(UGSM_ERR_NO_DEVICE, f"{path} not built: run `make -C ug_stereomatcher_amd/csrc`")
    if not _libs:
        _share_torch_hip_runtime(path)
    lib = C.CDLL(path)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    i = C.c_int
    lib.ugsm_default_config.argtypes = [C.POINTER(Config)]
    lib.ugsm_default_config.restype = None
    lib.ugsm_abi_version.restype = i
    lib.ugsm_is_dev_library.restype = i
    lib.ugsm_status_string.argtypes = [i]
    lib.ugsm_status_string.restype = C.c_char_p
    lib.ugsm_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.ugsm_destroy.argtypes = [vp]
    lib.ugsm_destroy.restype = None
    lib.ugsm_last_error.argtypes = [vp]
    lib.ugsm_last_error.restype = C.c_char_p
    lib.ugsm_level_dims.argtypes = [i, i, i, ip, ip]
    lib.ugsm_level_iterations.argtypes = [i]
    lib.ugsm_level_smooth_passes.argtypes = [i]
    lib.ugsm_threshold_schedule.argtypes = [i, fp]
    lib.ugsm_fovea_dims.argtypes = [i, i, i, i, ip, ip]
    lib.ugsm_pixel_iterations.argtypes = [i, i, i, i]
    lib.ugsm_pixel_iterations.restype = C.c_longlong
    lib.ugsm_plan_level.argtypes = [C.POINTER(Config), i, i, i, C.POINTER(LevelPlan)]
    lib.ugsm_match_full.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]
    lib.ugsm_submit_full_host.argtypes = [vp, i, vp, vp, i, i, i, vp, vp, vp]
    lib.ugsm_submit_foveated_host.argtypes = [vp, i, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp]
    lib.ugsm_match_foveated.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp]
    lib.ugsm_match_foveated_full.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp]
    lib.ugsm_submit_full.argtypes = [vp, i, vp, vp, i, i, i, vp]
    lib.ugsm_submit_foveated.argtypes = [vp, i, vp, vp, i, i, i, i, i, vp, vp, vp]
    pp = C.POINTER(vp)
    lib.ugsm_submit_full_batch.argtypes = [vp, i, i, pp, pp, i, i, i, pp]
    lib.ugsm_submit_foveated_batch.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, pp, pp]
    lib.ugsm_submit_full_batch_host.argtypes = [vp, i, i, pp, pp, i, i, i, pp, pp, pp]
    lib.ugsm_submit_foveated_batch_host.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, pp, pp]
    lib.ugsm_submit_foveated_multi.argtypes = [vp, i, vp, vp, i, i, i, i, ip, ip, pp]
    lib.ugsm_match_foveated_multi.argtypes = [vp, vp, vp, i, i, i, i, ip, ip, pp, pp, pp]
    lib.ugsm_reconstruct_full_multi.argtypes = [vp, i, i, pp, i, i, ip, ip, vp]
    lib.ugsm_submit_foveated_multi_checked.argtypes = [vp, i, vp, vp, i, i, i, i, ip, ip, pp, C.c_float]
    lib.ugsm_match_foveated_multi_checked.argtypes = [vp, vp, vp, i, i, i, i, ip, ip, pp, pp, pp, C.c_float]
    lib.ugsm_submit_full_checked.argtypes = [vp, i, i, pp, pp, i, i, i, pp, pp, C.c_float]
    lib.ugsm_match_full_checked.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, C.c_float]
    lib.ugsm_submit_full_checked_host.argtypes = [vp, i, i, pp, pp, i, i, i, pp, pp, pp, pp, pp, pp, C.c_float]
    lib.ugsm_last_lr_marked_pair.argtypes = [vp, i, i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.ugsm_submit_full_seeded.argtypes = [vp, i, i, pp, pp, i, i, i, pp, i, pp]
    lib.ugsm_match_full_seeded.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp]
    lib.ugsm_stage_restrict.argtypes = [vp, vp, i, i, i, vp]
    lib.ugsm_seeded_pixel_iterations.argtypes = [i, i, i, i]
    lib.ugsm_seeded_pixel_iterations.restype = C.c_longlong
    ip = C.POINTER(C.c_int)
    lib.ugsm_submit_foveated_warm.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, ip, ip, i, pp]
    lib.ugsm_submit_foveated_warm_field.argtypes = [vp, i, i, pp, pp, i, i, i, ip, ip, pp, i, pp]
    lib.ugsm_match_foveated_warm.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, i, i, i, vp, vp, vp]
    lib.ugsm_stage_warm_stack.argtypes = [vp, vp, i, i, i, i, i, i, i, vp]
    lib.ugsm_fovea_warm_pixel_iterations.argtypes = [i, i, i, i, i]
    lib.ugsm_fovea_warm_pixel_iterations.restype = C.c_longlong
    lib.ugsm_submit_full_coarse.argtypes = [vp, i, i, pp, pp, i, i, i, i, pp, pp]
    lib.ugsm_submit_full_fine.argtypes = [vp, i, i, pp, pp, i, i, i, pp, i, pp]
    lib.ugsm_match_full_coarse.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp]
    lib.ugsm_match_full_fine.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp]
    lib.ugsm_stage_prolong.argtypes = [vp, vp, i, i, i, vp]
    lib.ugsm_coarse_pixel_iterations.argtypes = [i, i, i, i]
    lib.ugsm_coarse_pixel_iterations.restype = C.c_longlong
    lib.ugsm_wait.argtypes = [vp, i]
    lib.ugsm_wait_all.argtypes = [vp]
    lib.ugsm_submit_pyramids.argtypes = [vp, i, vp, vp, i, i, i]
    lib.ugsm_submit_fovea_coarse.argtypes = [vp, i, vp]
    lib.ugsm_submit_fovea_fine.argtypes = [vp, i, vp, i, i, vp]
    lib.ugsm_triangulate.argtypes = [vp, i, vp, vp, i, i, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.ugsm_fovea_mapping.argtypes = [i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_float)]
    lib.ugsm_triangulate_fovea.argtypes = [vp, i, vp, vp, i, i, i, i, i, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.ugsm_reconstruct_full.argtypes = [vp, i, vp, vp, vp, i, i, i, i, vp]
    lib.ugsm_stage_pyramid.argtypes = [vp, vp, i, i, i, i, vp]
    lib.ugsm_stage_iterate.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, vp]
    lib.ugsm_stage_seed.argtypes = [vp, vp, i, i, vp, i, i, i, i, i, i]
    lib.ugsm_stage_smooth.argtypes = [vp, vp, i, i, i, i]
    if dev:
        lib.ugsm_stage_poly_probe.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i]
        lib.ugsm_stage_div3_probe.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i]
        lib.ugsm_stage_div_probe.argtypes = [vp, vp, vp, vp, i]
        lib.ugsm_stage_range_words.argtypes = [vp, i, C.POINTER(C.c_uint), i]
        lib.ugsm_stage_level0_direct.argtypes = [vp, i]
        lib.ugsm_stage_iterate_rgb8.argtypes = [vp, vp, vp, i, vp, i, i, i, i, i, i, i]
    lib.ugsm_stage_weighted_difference.argtypes = [vp, vp, vp, i, i, C.POINTER(C.c_float)]
    lib.ugsm_last_iterations.argtypes = [vp, i, C.POINTER(i)]
    lib.ugsm_stage_lr_check.argtypes = [vp, vp, vp, i, i, C.c_float, C.POINTER(C.c_longlong)]
    lib.ugsm_last_lr_marked.argtypes = [vp, i]
    lib.ugsm_last_lr_marked.restype = C.c_longlong
    lib.ugsm_set_lr_check.argtypes = [vp, C.c_float, i]
    lib.ugsm_get_lr_check.argtypes = [vp, C.POINTER(C.c_float), ip]
    lib.ugsm_last_lr_marked_levels.argtypes = [vp, i, i, C.POINTER(C.c_longlong)]
    lib.ugsm_slot_stream.argtypes = [vp, i, C.POINTER(vp)]
    lib.ugsm_get_kernel_stats.argtypes = [vp, C.POINTER(KernelStat), i]
    lib.ugsm_reset_kernel_stats.argtypes = [vp]
    lib.ugsm_set_profile_events.argtypes = [vp, i]
    lib.ugsm_dev_alloc.argtypes = [vp, C.POINTER(vp), C.c_longlong]
    lib.ugsm_dev_free.argtypes = [vp, vp]
    lib.ugsm_host_alloc.argtypes = [vp, C.POINTER(vp), C.c_longlong]
    lib.ugsm_host_free.argtypes = [vp, vp]
    lib.ugsm_copy_to_device.argtypes = [vp, vp, vp, C.c_longlong]
    lib.ugsm_copy_to_host.argtypes = [vp, vp, vp, C.c_longlong]
    u64 = C.c_uint64
    lib.ugsm_poll.argtypes = [vp, i]
    lib.ugsm_context_device_bytes.argtypes = [vp]
    lib.ugsm_context_device_bytes.restype = C.c_longlong
    lib.ugsm_enqueue_full.argtypes = [vp, vp, vp, i, i, i, vp, u64]
    lib.ugsm_enqueue_foveated.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, u64]
    lib.ugsm_enqueue_full_host.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, u64]
    lib.ugsm_enqueue_foveated_host.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, u64]
    lib.ugsm_enqueue_full_managed.argtypes = [vp, vp, vp, i, i, i, u64]
    lib.ugsm_enqueue_foveated_managed.argtypes = [vp, vp, vp, i, i, i, i, i, i, u64]
    lib.ugsm_enqueue_full_cloud.argtypes = [vp, vp, vp, i, i, i, vp, C.POINTER(QueueCloud), vp, C.c_longlong, vp, u64]
    lib.ugsm_enqueue_foveated_cloud.argtypes = [vp, vp, vp, i, i, i, i, i, vp, C.POINTER(QueueCloud), vp, C.c_longlong, vp, vp, u64]
    lib.ugsm_enqueue_full_cloud_managed.argtypes = [vp, vp, vp, i, i, i, C.POINTER(QueueCloud), u64]
    lib.ugsm_enqueue_foveated_cloud_managed.argtypes = [vp, vp, vp, i, i, i, i, i, C.POINTER(QueueCloud), u64]
    lib.ugsm_done_cloud.argtypes = [vp, C.POINTER(CloudResult)]
    lib.ugsm_enqueue_full_checked.argtypes = [vp, vp, vp, i, i, i, vp, vp, C.c_float, u64]
    lib.ugsm_enqueue_full_checked_managed.argtypes = [vp, vp, vp, i, i, i, C.c_float, i, u64]
    lib.ugsm_enqueue_full_checked_cloud.argtypes = [vp, vp, vp, i, i, i, vp, vp, C.c_float, C.POINTER(QueueCloud), vp, C.c_longlong, vp, u64]
    lib.ugsm_enqueue_full_checked_cloud_managed.argtypes = [vp, vp, vp, i, i, i, C.c_float, i, C.POINTER(QueueCloud), u64]
    lib.ugsm_done_checked.argtypes = [vp, C.POINTER(CheckedResult)]
    lib.ugsm_flush.argtypes = [vp]
    lib.ugsm_next_done.argtypes = [vp, C.POINTER(Completion), i]
    lib.ugsm_queue_depth.argtypes = [vp, ip, ip, ip]
    lib.ugsm_queue_plan.argtypes = [C.POINTER(Config), i, ip, i]
    lib.ugsm_shard_unique_id.argtypes = [vp]
    lib.ugsm_shard_init.argtypes = [vp, vp, i, i]
    lib.ugsm_shard_init_all.argtypes = [C.POINTER(vp), i]
    lib.ugsm_shard_rank.argtypes = [vp, ip, ip]
    lib.ugsm_shard_count_ranks.argtypes = [vp, ip]
    lib.ugsm_submit_fovea_shard.argtypes = [vp, i, vp, vp, i, i, i, i, i, vp, i]
    lib.ugsm_shard_set_timeout.argtypes = [vp, C.c_longlong]
    lib.ugsm_shard_gather.argtypes = [vp, i, vp, C.c_longlong, vp, i]
    lib.ugsm_shard_finalize.argtypes = [vp]
    lib.ugsm_input_bytes_per_pixel.argtypes = [i]
    lib.ugsm_input_format_from_encoding.argtypes = [C.c_char_p]
    lib.ugsm_set_input_format.argtypes = [vp, i]
    lib.ugsm_get_input_format.argtypes = [vp, ip]
    lib.ugsm_default_cloud_params.argtypes = [C.POINTER(CloudParams)]
    lib.ugsm_default_cloud_params.restype = None
    lib.ugsm_cloud_points.argtypes = [i, i, i]
    lib.ugsm_cloud_points.restype = C.c_longlong
    dpp = C.POINTER(C.c_double)
    lib.ugsm_point_cloud.argtypes = [vp, i, vp, vp, vp, vp, i, i, i, dpp, dpp, C.POINTER(CloudParams), vp, C.c_longlong, vp]
    lib.ugsm_point_cloud_fovea.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i, C.c_float, vp, i, i, i, dpp, dpp, C.POINTER(CloudParams), vp,
                                           C.c_longlong, vp]
    lib.ugsm_resized_cloud_points.argtypes = [i, i, C.c_float]
    lib.ugsm_resized_cloud_points.restype = C.c_longlong
    lib.ugsm_point_cloud_resized.argtypes = [vp, i, vp, vp, vp, vp, i, i, i, dpp, dpp, C.c_float, C.POINTER(CloudParams), vp, C.c_longlong, vp]
    lib.ugsm_point_cloud_resized_fovea.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i, C.c_float, vp, i, i, i, dpp, dpp, C.c_float, i,
                                                   C.POINTER(CloudParams), vp, C.c_longlong, vp]
    lib.ugsm_fovea_level_mapping.argtypes = [i, i, i, i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_float)]
    lib.ugsm_fovea_cloud_points.argtypes = [i, i, i, i, i, i, i, C.POINTER(C.c_longlong)]
    lib.ugsm_fovea_cloud_points.restype = C.c_longlong
    lib.ugsm_point_cloud_fovea_all.argtypes = [vp, i, vp, vp, vp, i, i, i, i, vp, i, dpp, dpp, C.POINTER(CloudParams), vp, C.c_longlong, vp, vp]
    lib.ugsm_fovea_multi_cloud_points.argtypes = [i, i, i, i, i, ip, ip, i, C.POINTER(C.c_longlong)]
    lib.ugsm_fovea_multi_cloud_points.restype = C.c_longlong
    lib.ugsm_point_cloud_fovea_multi.argtypes = [vp, i, i, pp, i, i, ip, ip, vp, i, dpp, dpp, C.POINTER(CloudParams), vp, C.c_longlong, vp, vp]
    lib.ugsm_warp_planes.argtypes = [vp, i, vp, i, i, i, vp, vp, vp]
    lib.ugsm_warp_right.argtypes = [vp, i, vp, i, i, i, vp, vp, vp]
    lib.ugsm_warp_right_fovea.argtypes = [vp, i, vp, vp, vp, i, i, vp]
    lib.ugsm_photometric_residual.argtypes = [vp, i, vp, vp, i, i, i, vp, vp, vp, vp]
    lib.ugsm_photometric_residual_fovea.argtypes = [vp, i, vp, vp, vp, vp, vp, i, i, vp]
    lib.ugsm_default_depth_params.argtypes = [C.POINTER(DepthParams)]
    lib.ugsm_default_depth_params.restype = None
    lib.ugsm_depth_image_size.argtypes = [i, i, C.c_float, ip, ip]
    lib.ugsm_depth_image.argtypes = [vp, i, vp, vp, vp, i, i, dpp, dpp, C.POINTER(DepthParams), vp, vp]
    lib.ugsm_depth_image_fovea.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i, dpp, dpp, C.POINTER(DepthParams), vp, vp]
    lib.ugsm_match_full_depth.argtypes = [vp, vp, vp, i, i, i, dpp, dpp, C.POINTER(DepthParams), vp, vp, vp, vp]
    lib.ugsm_depth_image_fovea_full.argtypes = [vp, i, vp, vp, vp, i, i, i, i, dpp, dpp, C.POINTER(DepthParams), vp, vp]
    lib.ugsm_depth_image_fovea_multi.argtypes = [vp, i, i, C.POINTER(vp), i, i, C.POINTER(i), C.POINTER(i), dpp, dpp, C.POINTER(DepthParams), vp, vp]
    lib.ugsm_match_foveated_depth.argtypes = [vp, vp, vp, i, i, i, i, i, dpp, dpp, C.POINTER(DepthParams), vp, vp, vp, vp]
    lib.ugsm_set_lens.argtypes = [vp, dpp, dpp, dpp, dpp, i]
    lib.ugsm_get_lens.argtypes = [vp, dpp, dpp, dpp, dpp, ip, ip]
    lib.ugsm_undistort_points.argtypes = [dpp, dpp, i, vp, vp, C.c_longlong]
    if bool(lib.ugsm_is_dev_library()) != bool(dev):
        raise UgsmError(UGSM_ERR_STATE, f"{path} is not the {'development' if dev else 'product'} build")
    _libs[dev] = lib
    return lib


def status_string(st: int) -> str:
    return load().ugsm_status_string(st).decode()


# ---- pure-host geometry (no GPU needed) -------------------------------------------------

def level_dims(W: int, H: int, levels: int = 14):
    w = (C.c_int * UGSM_MAX_LEVELS)()
    h = (C.c_int * UGSM_MAX_LEVELS)()
    st = load().ugsm_level_dims(W, H, levels, w, h)
    if st:
        raise UgsmError(st, status_string(st))
    return list(w[:levels]), list(h[:levels])


def level_iterations(level: int) -> int:
    return load().ugsm_level_iterations(level)


def level_smooth_passes(level: int) -> int:
    return load().ugsm_level_smooth_passes(level)


def threshold_schedule(mi: int) -> np.ndarray:
    out = np.zeros(mi, np.float32)
    st = load().ugsm_threshold_schedule(mi, out.ctypes.data_as(C.POINTER(C.c_float)))
    if st:
        raise UgsmError(st, status_string(st))
    return out


def fovea_dims(W: int, H: int, levels: int = 14, fovea_levels: int = 7):
    fw, fh = C.c_int(), C.c_int()
    st = load().ugsm_fovea_dims(W, H, levels, fovea_levels, C.byref(fw), C.byref(fh))
    if st:
        raise UgsmError(st, status_string(st))
    return fw.value, fh.value


def pixel_iterations(W: int, H: int, levels: int = 14, fovea_levels: int = 0) -> int:
    return int(load().ugsm_pixel_iterations(W, H, levels, fovea_levels))


def seeded_pixel_iterations(W: int, H: int, levels: int = 14, start_level: int = 0) -> int:
    """Sum of iterations x pixels over the levels start_level .. 0: what a seeded full-mode call runs (-1: no such size or level)."""
    return int(load().ugsm_seeded_pixel_iterations(W, H, levels, start_level))


def coarse_pixel_iterations(W: int, H: int, levels: int = 14, stop_level: int = 0) -> int:
    """Sum of iterations x pixels over the levels stop_level .. levels - 1: what the coarse half of a full-mode call runs (-1: no such size or level)."""
    return int(load().ugsm_coarse_pixel_iterations(W, H, levels, stop_level))


def fovea_warm_pixel_iterations(W: int, H: int, levels: int = 14, fovea_levels: int = 7, start_level: int = 0) -> int:
    """fovW x fovH x the iterations of the levels start_level .. 0: what a warm foveated call runs (-1: no such size or level)."""
    return int(load().ugsm_fovea_warm_pixel_iterations(W, H, levels, fovea_levels, start_level))


def cloud_params(sampling: int = 1, format: int = UGSM_CLOUD_PCL32, compact: bool = False, min_conf: float | None = None,
                 z_min: float | None = None, z_max: float | None = None) -> CloudParams:
    """ugsm_cloud_params from ugsm_default_cloud_params with the named fields changed (None: the default)."""
    p = CloudParams()
    load().ugsm_default_cloud_params(C.byref(p))
    p.sampling, p.format, p.compact = int(sampling), int(format), int(bool(compact))
    for name, v in (("min_conf", min_conf), ("z_min", z_min), ("z_max", z_max)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def depth_params(format: int = UGSM_DEPTH_32F, unit: float | None = None, min_conf: float | None = None, z_min: float | None = None,
                 z_max: float | None = None, factor: float | None = None) -> DepthParams:
    """ugsm_depth_params from ugsm_default_depth_params with the named fields changed (None: the default)."""
    p = DepthParams()
    load().ugsm_default_depth_params(C.byref(p))
    p.format = int(format)
    for name, v in (("unit", unit), ("min_conf", min_conf), ("z_min", z_min), ("z_max", z_max), ("factor", factor)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def _doubles(a, n: int, what: str):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size != n:
        raise UgsmError(UGSM_ERR_BAD_ARG, f"{what}: {n} values")
    return (C.c_double * n)(*a)


def undistort_points(K, D, uv, iterations: int = 5) -> np.ndarray:
    """The lens definition of include/ugsm.h on the host (ugsm_undistort_points; no context, no device): uv of shape (..., 2), float32 pixel
    coordinates (u, v) under K (3 x 3) and D = (k1, k2, p1, p2, k3); returns the undistorted coordinates in the same shape."""
    src = np.ascontiguousarray(uv, np.float32)
    if src.ndim < 1 or src.shape[-1] != 2:
        raise UgsmError(UGSM_ERR_BAD_ARG, "undistort_points: uv of shape (..., 2)")
    dst = np.empty_like(src)
    st = load().ugsm_undistort_points(_doubles(K, 9, "K"), _doubles(D, 5, "D"), int(iterations), src.ctypes.data, dst.ctypes.data, src.size // 2)
    if st != UGSM_OK:
        raise UgsmError(st, "ugsm_undistort_points")
    return dst


def depth_image_size(pw: int, ph: int, factor: float = 1.0):
    """(dw, dh) of the depth image of pw x ph planes, the resized clouds' rule with f a float32; None on bad arguments."""
    dw, dh = C.c_int(), C.c_int()
    if load().ugsm_depth_image_size(pw, ph, C.c_float(float(factor)), C.byref(dw), C.byref(dh)):
        return None
    return dw.value, dh.value


def cloud_points(W: int, H: int, sampling: int = 1) -> int:
    """Points of the dense cloud, ceil(W / s) * ceil(H / s); -1 on bad arguments."""
    return int(load().ugsm_cloud_points(W, H, sampling))


def resized_cloud_points(W: int, H: int, factor: float) -> int:
    """Points of the resized cloud, (int)((float)W * f) * (int)((float)H * f) with f a float32; -1 on bad arguments."""
    return int(load().ugsm_resized_cloud_points(W, H, C.c_float(float(factor))))


def fovea_level_mapping(W: int, H: int, levels: int, fovea_levels: int, src_level: int, off=(0, 0)):
    """ugsm_fovea_mapping(.., src_level, 0) for any fovea_levels and window offset -> (left_margin, upper_margin, scale); host only."""
    l, u, sc = C.c_int(), C.c_int(), C.c_float()
    st = load().ugsm_fovea_level_mapping(W, H, levels, fovea_levels, int(off[0]), int(off[1]), src_level, C.byref(l), C.byref(u), C.byref(sc))
    if st:
        raise UgsmError(st, "ugsm_fovea_level_mapping")
    return l.value, u.value, np.float32(sc.value)


def fovea_cloud_points(W: int, H: int, levels: int = 14, fovea_levels: int = 7, off=(0, 0), sampling: int = 1, per_level: bool = False):
    """Points of the dense merged cloud of the fovea stack (ugsm_point_cloud_fovea_all), -1 on bad arguments; with per_level, also the
    list of each level's points."""
    per = (C.c_longlong * UGSM_MAX_LEVELS)()
    n = int(load().ugsm_fovea_cloud_points(W, H, levels, fovea_levels, int(off[0]), int(off[1]), sampling, per))
    return (n, list(per[:fovea_levels]) if n >= 0 else []) if per_level else n


def fovea_multi_cloud_points(W: int, H: int, levels: int, fovea_levels: int, offsets, sampling: int = 1, per_entry: bool = False):
    """Points of the dense merged cloud of the stacks of len(offsets) windows of one pair (ugsm_point_cloud_fovea_multi), -1 on bad
    arguments; with per_entry, also the list of each entry's points, level-major: (fovea_levels - 1) * len(offsets) + 1 entries."""
    n = len(offsets)
    E = max((fovea_levels - 1) * n + 1, 1)
    per = (C.c_longlong * E)()
    ox, oy = (C.c_int * n)(*[int(o[0]) for o in offsets]), (C.c_int * n)(*[int(o[1]) for o in offsets])
    total = int(load().ugsm_fovea_multi_cloud_points(W, H, levels, fovea_levels, n, ox, oy, sampling, per))
    return (total, list(per[:E]) if total >= 0 else []) if per_entry else total


def input_bytes_per_pixel(format: int) -> int:
    """3, 3, 4, 4, 1 for UGSM_INPUT_RGB8 .. UGSM_INPUT_MONO8, 12 and 4 for UGSM_INPUT_RGB32F and UGSM_INPUT_MONO32F (INPUT_BYTES_PER_PIXEL);
    -1 for an unknown format."""
    return int(load().ugsm_input_bytes_per_pixel(int(format)))


def input_format_from_encoding(encoding) -> int:
    """The UGSM_INPUT_* of a sensor_msgs encoding name (INPUT_ENCODINGS: "rgb8", "bgr8", "rgba8", "bgra8", "mono8", "32FC3", "32FC1"); -1 for any
    other (and None)."""
    if isinstance(encoding, str):
        encoding = encoding.encode()
    return int(load().ugsm_input_format_from_encoding(encoding))


# ---- context -----------------------------------------------------------------------------

class Context:
    """Owns a ugsm_ctx*.  One per device; calls must be serialised by the caller."""

    def __init__(self, device: int = 0, levels: int = 14, fovea_levels: int = 7, slots: int = 1,
                 kernel_path: int = 0, profile_events: int = 0, march_min_pixels: int = 0, march_np: int = 0,
                 march_rows: int = 0, march_smooth: int = 0, early_exit_threshold: float = 0.0, small_max_pixels: int = 0,
                 lr_check_threshold: float = 0.0, streams: int = 0, batch: int = 0, stream_priority: int = 0, dev: bool | None = None):
        # libugsm_dev.so when asked for, or when the configuration needs a kernel only it has
        self.dev = bool(dev) if dev is not None else (kernel_path == 1 or march_min_pixels < 0)
        lib = load(self.dev)
        cfg = Config()
        lib.ugsm_default_config(C.byref(cfg))
        # full-mode users never name fovea_levels; keep the default legal for short pyramids
        cfg.device, cfg.levels, cfg.fovea_levels, cfg.slots = device, levels, min(fovea_levels, levels), slots
        cfg.kernel_path, cfg.profile_events = kernel_path, int(profile_events)
        cfg.march_min_pixels, cfg.march_np, cfg.march_rows = int(march_min_pixels), int(march_np), int(march_rows)
        cfg.march_smooth = int(march_smooth)
        cfg.early_exit_threshold = float(early_exit_threshold)
        cfg.small_max_pixels = int(small_max_pixels)
        cfg.lr_check_threshold = float(lr_check_threshold)
        cfg.streams = int(streams)
        cfg.batch, cfg.stream_priority = int(batch), int(stream_priority)
        self.cfg = cfg
        self._pinned = []
        self._h = C.c_void_p()
        st = lib.ugsm_create(C.byref(cfg), C.byref(self._h))
        if st:
            self._h = None
            raise UgsmError(st, status_string(st) + " (libugsm needs a HIP device; there is no CPU fallback)")
        self.lib = lib

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self.lib.ugsm_host_free(self._h, p)
            self._pinned = []
            if getattr(self, "_res_sums", None) is not None:
                self.lib.ugsm_dev_free(self._h, self._res_sums)
                self._res_sums = None
            self.lib.ugsm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, st: int):
        if st:
            raise UgsmError(st, f"{status_string(st)}: {self.lib.ugsm_last_error(self._h).decode()}")

    @property
    def handle(self):
        return self._h

    # ---- input format (ugsm_set_input_format): captured by every call that hands an image over --------------------------------------
    def set_input_format(self, format: int):
        self.check(self.lib.ugsm_set_input_format(self._h, int(format)))

    @property
    def input_format(self) -> int:
        f = C.c_int()
        self.check(self.lib.ugsm_get_input_format(self._h, C.byref(f)))
        return f.value

    # ---- the LR check (ugsm_set_lr_check): captured by every slot-level call; fixed while the queue holds pairs ----------------------------
    def set_lr_check(self, tau: float, modes: int = UGSM_LR_FULL | UGSM_LR_FOVEATED):
        self.check(self.lib.ugsm_set_lr_check(self._h, float(tau), int(modes)))

    @property
    def lr_check(self):
        """(tau, modes)"""
        tau, modes = C.c_float(), C.c_int()
        self.check(self.lib.ugsm_get_lr_check(self._h, C.byref(tau), C.byref(modes)))
        return tau.value, modes.value

    # ---- lens distortion (ugsm_set_lens): read by every triangulation, cloud and depth call when it is made ------------------------------
    def set_lens(self, K1, D1, K2, D2, iterations: int = 5):
        """K (3 x 3) and D = (k1, k2, p1, p2, k3) of the left and the right camera, as sensor_msgs/CameraInfo holds them."""
        self.check(self.lib.ugsm_set_lens(self._h, _doubles(K1, 9, "K1"), _doubles(D1, 5, "D1"), _doubles(K2, 9, "K2"), _doubles(D2, 5, "D2"),
                                          int(iterations)))

    def clear_lens(self):
        self.check(self.lib.ugsm_set_lens(self._h, None, None, None, None, 0))

    def get_lens(self):
        """None while no lens is set, else (K1, D1, K2, D2, iterations) with K of shape (3, 3)."""
        K1, K2, D1, D2 = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_double * 5)(), (C.c_double * 5)()
        it, on = C.c_int(), C.c_int()
        self.check(self.lib.ugsm_get_lens(self._h, K1, D1, K2, D2, C.byref(it), C.byref(on)))
        if not on.value:
            return None
        return np.array(K1).reshape(3, 3), np.array(D1), np.array(K2).reshape(3, 3), np.array(D2), it.value

    def last_lr_marked(self, slot: int = 0) -> int:
        return int(self.lib.ugsm_last_lr_marked(self._h, slot))

    def last_lr_marked_levels(self, slot: int = 0, pair: int = 0):
        """Pixels the foveated check marked on each level (0 = finest first) of pair `pair` of the last call on `slot`."""
        out = (C.c_longlong * UGSM_MAX_LEVELS)()
        self.check(self.lib.ugsm_last_lr_marked_levels(self._h, slot, pair, out))
        return [int(v) for v in out[:self.cfg.fovea_levels]]

    def check_image(self, a: np.ndarray):
        """(H, W) uint8 for mono8, (H, W, 3) for rgb8 / bgr8, (H, W, 4) for rgba8 / bgra8, (H, W, 3) float32 for rgb32f, (H, W) float32 for mono32f,
        matching the context's input format; rows may be padded (a view of a wider array), pixels must be contiguous.  Returns (W, H, stride)."""
        bpp = input_bytes_per_pixel(self.input_format)
        size = 4 if self.input_format in (UGSM_INPUT_RGB32F, UGSM_INPUT_MONO32F) else 1  # bytes per sample
        ch = bpp // size
        if a.dtype != (np.float32 if size == 4 else np.uint8) or not ((a.ndim == 2 and ch == 1) or (a.ndim == 3 and a.shape[2] == ch and ch > 1)):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, f"image of shape {a.shape} and dtype {a.dtype} does not match the input format "
                                                    f"{self.input_format} ({bpp} bytes per pixel)")
        if (a.ndim == 3 and a.strides[1:] != (bpp, size)) or (a.ndim == 2 and a.strides[1] != size):
            raise UgsmError(UGSM_ERR_BAD_ARG, "image pixels must be contiguous")
        return a.shape[1], a.shape[0], a.strides[0]

    # device memory through the C-ABI (tests / C hosts); bench.py uses torch tensors instead
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self.check(self.lib.ugsm_dev_alloc(self._h, C.byref(p), nbytes))
        return p.value

    def free(self, ptr: int):
        self.check(self.lib.ugsm_dev_free(self._h, ptr))

    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.check(self.lib.ugsm_copy_to_device(self._h, p, arr.ctypes.data, arr.nbytes))
        return p

    def to_host(self, ptr: int, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype)
        self.check(self.lib.ugsm_copy_to_host(self._h, out.ctypes.data, ptr, out.nbytes))
        return out

    def host_array(self, shape, dtype=np.float32) -> np.ndarray:
        """A numpy array in page-locked host memory (ugsm_host_alloc); freed when the context closes."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self.check(self.lib.ugsm_host_alloc(self._h, C.byref(p), nbytes))
        self._pinned.append(p.value)
        buf = (C.c_char * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def triangulate(self, d_dispx: int, d_dispy: int, W: int, H: int, P1, P2, d_xyz: int, slot: int = 0):
        """SURVEY 8f row f-1 (getPointCloud.cpp:886-949): X, Y, Z planes from device (dx, dy) planes."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_triangulate(self._h, slot, d_dispx, d_dispy, W, H, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), d_xyz))
        self.check(self.lib.ugsm_wait(self._h, slot))

    def triangulate_fovea(self, d_stackx: int, d_stacky: int, fovW: int, fovH: int, src_level: int, left: int, upper: int, scale,
                          P1, P2, d_xyz: int, slot: int = 0):
        """Row f-1, foveated branch (getPointCloud.cpp:892-903): X, Y, Z planes for one level of the fovea stacks."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_triangulate_fovea(self._h, slot, d_stackx, d_stacky, fovW, fovH, src_level, left, upper,
                                                   C.c_float(float(scale)), p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), d_xyz))
        self.check(self.lib.ugsm_wait(self._h, slot))

    def point_cloud(self, d_dispx: int, d_dispy: int, d_conf, d_rgbL: int, W: int, H: int, stride: int, P1, P2, params: CloudParams,
                    d_points: int, cap_points: int, d_count: int, slot: int = 0) -> int:
        """Row f-1, the coloured cloud (getPointCloud.cpp doReconstructionRGB, :675-722) into d_points; waits on the slot and returns the
        cloud's number of points (which may exceed cap_points: only the first cap_points records are written)."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud(self._h, slot, d_dispx, d_dispy, d_conf, d_rgbL, W, H, stride, p1.ctypes.data_as(dp),
                                             p2.ctypes.data_as(dp), C.byref(params), d_points, int(cap_points), d_count))
        self.check(self.lib.ugsm_wait(self._h, slot))
        return int(self.to_host(d_count, (1,), np.int64)[0])

    def point_cloud_fovea(self, d_stackx: int, d_stacky: int, d_stackc, fovW: int, fovH: int, src_level: int, left: int, upper: int, scale,
                          d_rgbL: int, W: int, H: int, stride: int, P1, P2, params: CloudParams, d_points: int, cap_points: int, d_count: int,
                          slot: int = 0) -> int:
        """Row f-1, the foveated cloud (doReconstructionRGB_FOV, :615-673) of level src_level of the stacks; waits, returns the count."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud_fovea(self._h, slot, d_stackx, d_stacky, d_stackc, fovW, fovH, src_level, left, upper,
                                                   C.c_float(float(scale)), d_rgbL, W, H, stride, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp),
                                                   C.byref(params), d_points, int(cap_points), d_count))
        self.check(self.lib.ugsm_wait(self._h, slot))
        return int(self.to_host(d_count, (1,), np.int64)[0])

    def point_cloud_fovea_all(self, d_stackx: int, d_stacky: int, d_stackc, W: int, H: int, off, d_rgbL: int, stride: int, P1, P2,
                              params: CloudParams, d_points: int, cap_points: int, d_count: int, d_level_counts=None, slot: int = 0):
        """The whole fovea stack as one cloud (ugsm_point_cloud_fovea_all): level 0, then 1 .. F-1 without the pixels the finer level
        covers; waits on the slot and returns the count, or (count, per-level counts) when d_level_counts is given."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud_fovea_all(self._h, slot, d_stackx, d_stacky, d_stackc, W, H, int(off[0]), int(off[1]), d_rgbL,
                                                       stride, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), C.byref(params), d_points,
                                                       int(cap_points), d_count, d_level_counts))
        self.check(self.lib.ugsm_wait(self._h, slot))
        n = int(self.to_host(d_count, (1,), np.int64)[0])
        if d_level_counts is None:
            return n
        return n, self.to_host(d_level_counts, (self.cfg.fovea_levels,), np.int64).tolist()

    def point_cloud_fovea_multi(self, d_stacks, W: int, H: int, offsets, d_rgbL: int, stride: int, P1, P2, params: CloudParams, d_points: int,
                                cap_points: int, d_count: int, d_entry_counts=None, slot: int = 0):
        """The stacks of several windows of one pair as one cloud (ugsm_point_cloud_fovea_multi): the entries level-major, each without
        the pixels a finer level of any window or the same level of a higher-numbered window holds.  d_stacks: one device stack per window;
        offsets: one (off_x, off_y) per window, or None (all centred).  Waits on the slot and returns the count, or (count, per-entry
        counts) when d_entry_counts is given."""
        n = len(d_stacks)
        ox, oy = self._offsets(offsets, n)
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud_fovea_multi(self._h, slot, n, self._ptrs(d_stacks), W, H, ox, oy, d_rgbL, stride,
                                                         p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), C.byref(params), d_points,
                                                         int(cap_points), d_count, d_entry_counts))
        self.check(self.lib.ugsm_wait(self._h, slot))
        count = int(self.to_host(d_count, (1,), np.int64)[0])
        if d_entry_counts is None:
            return count
        return count, self.to_host(d_entry_counts, ((self.cfg.fovea_levels - 1) * n + 1,), np.int64).tolist()

    def point_cloud_resized(self, d_dispx: int, d_dispy: int, d_conf, d_rgbL: int, W: int, H: int, stride: int, P1, P2, factor: float,
                            params: CloudParams, d_points: int, cap_points: int, d_count: int, slot: int = 0) -> int:
        """Row f-1, the resized cloud (getPointCloud.cpp doReconstruction_resized, :724-800): the Z plane cubic-resized by `factor` (a
        float32), X, Y and colour at ((int)(ii / f), (int)(jj / f)); waits on the slot and returns the cloud's number of points."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud_resized(self._h, slot, d_dispx, d_dispy, d_conf, d_rgbL, W, H, stride, p1.ctypes.data_as(dp),
                                                     p2.ctypes.data_as(dp), C.c_float(float(factor)), C.byref(params), d_points,
                                                     int(cap_points), d_count))
        self.check(self.lib.ugsm_wait(self._h, slot))
        return int(self.to_host(d_count, (1,), np.int64)[0])

    def point_cloud_resized_fovea(self, d_stackx: int, d_stacky: int, d_stackc, fovW: int, fovH: int, src_level: int, left: int, upper: int,
                                  scale, d_rgbL: int, W: int, H: int, stride: int, P1, P2, factor: float, params: CloudParams, d_points: int,
                                  cap_points: int, d_count: int, colour_mapped: bool = False, slot: int = 0) -> int:
        """Row f-1, the resized foveated cloud (doReconstructionFOV_resized, :802-884) of level src_level of the stacks; the colour at the
        unmapped (xx, yy) as the reference reads it, or at the mapped pixel with colour_mapped.  Waits, returns the count."""
        p1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        self.check(self.lib.ugsm_point_cloud_resized_fovea(self._h, slot, d_stackx, d_stacky, d_stackc, fovW, fovH, src_level, left, upper,
                                                           C.c_float(float(scale)), d_rgbL, W, H, stride, p1.ctypes.data_as(dp),
                                                           p2.ctypes.data_as(dp), C.c_float(float(factor)), int(bool(colour_mapped)),
                                                           C.byref(params), d_points, int(cap_points), d_count))
        self.check(self.lib.ugsm_wait(self._h, slot))
        return int(self.to_host(d_count, (1,), np.int64)[0])

    # ---- the depth image, REP 118 32FC1 / 16UC1 (include/ugsm.h) ---------------------------------------------------------------------------
    @staticmethod
    def _proj(P1, P2):
        dp = C.POINTER(C.c_double)
        p1, p2 = np.ascontiguousarray(P1, np.float64).reshape(12), np.ascontiguousarray(P2, np.float64).reshape(12)
        return p1, p2, p1.ctypes.data_as(dp), p2.ctypes.data_as(dp)

    def depth_image(self, d_dispx: int, d_dispy: int, d_conf, W: int, H: int, P1, P2, params: DepthParams, d_depth: int, d_valid=None,
                    slot: int = 0, wait: bool = True):
        """The depth image of a full-resolution match into d_depth (dw x dh elements, depth_image_size); with d_valid and wait, returns the
        number of valid pixels stored."""
        p1, p2, q1, q2 = self._proj(P1, P2)
        self.check(self.lib.ugsm_depth_image(self._h, slot, d_dispx, d_dispy, d_conf, W, H, q1, q2, C.byref(params), d_depth, d_valid))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))
            if d_valid is not None:
                return int(self.to_host(d_valid, (1,), np.uint64)[0])

    def depth_image_fovea(self, d_stackx: int, d_stacky: int, d_stackc, W: int, H: int, off, level: int, P1, P2, params: DepthParams,
                          d_depth: int, d_valid=None, slot: int = 0, wait: bool = True):
        """The depth image of level `level` of the fovea stacks of a foveated call on a W x H frame at window offset `off`, or with
        UGSM_DEPTH_ALL_LEVELS of every level (level 0 first) in one launch; with d_valid and wait, returns the list of per-level counts."""
        p1, p2, q1, q2 = self._proj(P1, P2)
        self.check(self.lib.ugsm_depth_image_fovea(self._h, slot, d_stackx, d_stacky, d_stackc, W, H, int(off[0]), int(off[1]), int(level), q1,
                                                   q2, C.byref(params), d_depth, d_valid))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))
            if d_valid is not None:
                n = self.cfg.fovea_levels if level == UGSM_DEPTH_ALL_LEVELS else 1
                return self.to_host(d_valid, (n,), np.uint64).astype(np.int64).tolist()

    def match_full_depth(self, L: np.ndarray, R: np.ndarray, P1, P2, params: DepthParams, planes: bool = False):
        """The blocking call: the match of (L, R) and its depth image, a (dh, dw) float32 or uint16 array; with planes, also the match's
        (3, H, W) result -- otherwise only the image crosses the bus."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "left and right images differ in size or stride")
        size = depth_image_size(W, H, params.factor)
        if size is None or params.format not in DEPTH_DTYPES:
            raise UgsmError(UGSM_ERR_BAD_ARG, "depth parameters")
        p1, p2, q1, q2 = self._proj(P1, P2)
        depth = np.empty((size[1], size[0]), DEPTH_DTYPES[params.format])
        out = np.empty((3, H, W), np.float32) if planes else None
        ptr = [out[k].ctypes.data for k in range(3)] if planes else [None] * 3
        self.check(self.lib.ugsm_match_full_depth(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, q1, q2, C.byref(params),
                                                  depth.ctypes.data, *ptr))
        return (depth, out) if planes else depth

    def depth_image_fovea_full(self, d_stackx: int, d_stacky: int, d_stackc, W: int, H: int, off, P1, P2, params: DepthParams, d_depth: int,
                               d_valid=None, slot: int = 0, wait: bool = True):
        """The depth image of the WHOLE W x H frame from the fovea stacks of a foveated call at window offset `off` -- what reconstruct_full
        followed by depth_image gives, in one launch and without the field; with d_valid and wait, returns the number of valid pixels."""
        p1, p2, q1, q2 = self._proj(P1, P2)
        self.check(self.lib.ugsm_depth_image_fovea_full(self._h, slot, d_stackx, d_stacky, d_stackc, W, H, int(off[0]), int(off[1]), q1, q2,
                                                        C.byref(params), d_depth, d_valid))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))
            if d_valid is not None:
                return int(self.to_host(d_valid, (1,), np.uint64)[0])

    def depth_image_fovea_multi(self, d_stack, W: int, H: int, offsets, P1, P2, params: DepthParams, d_depth: int, d_valid=None, slot: int = 0,
                                wait: bool = True):
        """The same from the stacks of several windows of one pair (d_stack: their device addresses; offsets None: centred) -- what
        reconstruct_full_multi followed by depth_image gives: where windows overlap the highest index wins."""
        n = len(d_stack)
        ox, oy = self._offsets(offsets, n)
        p1, p2, q1, q2 = self._proj(P1, P2)
        self.check(self.lib.ugsm_depth_image_fovea_multi(self._h, slot, n, self._ptrs(d_stack), W, H, ox, oy, q1, q2, C.byref(params), d_depth,
                                                         d_valid))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))
            if d_valid is not None:
                return int(self.to_host(d_valid, (1,), np.uint64)[0])

    def match_foveated_depth(self, L: np.ndarray, R: np.ndarray, P1, P2, params: DepthParams, off=(0, 0), stack: bool = False):
        """The blocking call: the foveated match of (L, R) at window offset `off` and the depth image of the whole frame from its stack, a
        (dh, dw) float32 or uint16 array; with stack, also the (3, F, fovH, fovW) stack -- otherwise only the image crosses the bus."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "left and right images differ in size or stride")
        size = depth_image_size(W, H, params.factor)
        if size is None or params.format not in DEPTH_DTYPES:
            raise UgsmError(UGSM_ERR_BAD_ARG, "depth parameters")
        p1, p2, q1, q2 = self._proj(P1, P2)
        depth = np.empty((size[1], size[0]), DEPTH_DTYPES[params.format])
        out = None
        if stack:
            fw, fh = fovea_dims(W, H, self.cfg.levels, self.cfg.fovea_levels)
            out = np.empty((3, self.cfg.fovea_levels, fh, fw), np.float32)
        ptr = [out[k].ctypes.data for k in range(3)] if stack else [None] * 3
        self.check(self.lib.ugsm_match_foveated_depth(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, int(off[0]), int(off[1]), q1, q2,
                                                      C.byref(params), depth.ctypes.data, *ptr))
        return (depth, out) if stack else depth

    # ---- the warped right image and the photometric residual of a match (include/ugsm.h) -----------------------------------------------
    def warp_planes(self, d_src: int, channels: int, W: int, H: int, d_dispx: int, d_dispy: int, d_dst: int, slot: int = 0, wait: bool = True):
        """MatchGPULib::warpRightImage on device memory: `channels` float planes of W x H warped by one (dx, dy) into d_dst."""
        self.check(self.lib.ugsm_warp_planes(self._h, slot, d_src, channels, W, H, d_dispx, d_dispy, d_dst))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))

    def warp_right(self, d_rgbR: int, W: int, H: int, stride: int, d_dispx: int, d_dispy: int, d_warp3: int, slot: int = 0, wait: bool = True):
        """The right image (the context's input format) warped into three float planes at d_warp3; wait=False leaves it on the slot's stream."""
        self.check(self.lib.ugsm_warp_right(self._h, slot, d_rgbR, W, H, stride, d_dispx, d_dispy, d_warp3))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))

    def warp_right_fovea(self, d_pyrR: int, d_stackx: int, d_stacky: int, fovW: int, fovH: int, d_warp: int, slot: int = 0, wait: bool = True):
        """Every level of the right fovea pyramid stack warped by its level of the disparity stacks, one launch; d_warp laid out as d_pyrR."""
        self.check(self.lib.ugsm_warp_right_fovea(self._h, slot, d_pyrR, d_stackx, d_stacky, fovW, fovH, d_warp))
        if wait:
            self.check(self.lib.ugsm_wait(self._h, slot))

    def _residual_sums(self, levels: int, slot: int):
        """The doubles the last residual on `slot` wrote -> (S / C as float32[levels][3], C[levels]); the raw sums stay in last_residual_sums."""
        self.check(self.lib.ugsm_wait(self._h, slot))
        raw = self.to_host(self._res_sums, (levels, 4), np.float64)
        self.last_residual_sums = raw
        with np.errstate(all="ignore"):
            q = (raw[:, :3] / raw[:, 3:4]).astype(np.float32)
        return q, raw[:, 3].copy()

    def _residual_buffer(self):
        if getattr(self, "_res_sums", None) is None:
            self._res_sums = self.alloc(UGSM_MAX_LEVELS * 4 * 8)   # (freed by close())
        return self._res_sums

    def photometric_residual(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, d_dispx: int, d_dispy: int, d_conf=None, slot: int = 0):
        """sum(|L_c - warp(R_c)| * conf) / sum(conf) per channel, straight from the two images: (float32[3], C); the four raw doubles
        S_0, S_1, S_2, C are kept in last_residual_sums[0].  d_conf None: every weight 1."""
        self.check(self.lib.ugsm_photometric_residual(self._h, slot, d_rgbL, d_rgbR, W, H, stride, d_dispx, d_dispy, d_conf, self._residual_buffer()))
        q, c = self._residual_sums(1, slot)
        return q[0], float(c[0])

    def photometric_residual_fovea(self, d_pyrL: int, d_pyrR: int, d_stackx: int, d_stacky: int, d_stackc, fovW: int, fovH: int, slot: int = 0):
        """The same per level of a fovea stack: (float32[F][3], C[F]); the raw doubles [level][S_0, S_1, S_2, C] in last_residual_sums."""
        self.check(self.lib.ugsm_photometric_residual_fovea(self._h, slot, d_pyrL, d_pyrR, d_stackx, d_stacky, d_stackc, fovW, fovH,
                                                            self._residual_buffer()))
        return self._residual_sums(self.cfg.fovea_levels, slot)

    def cloud_to_host(self, d_points: int, count: int, format: int = UGSM_CLOUD_PCL32) -> np.ndarray:
        """The first `count` records at d_points as a structured array of CLOUD_PCL32 or CLOUD_XYZRGB16."""
        if int(count) == 0:
            return np.empty(0, CLOUD_DTYPES[format])
        return self.to_host(d_points, (int(count),), CLOUD_DTYPES[format])

    def reconstruct_full(self, d_stackH: int, d_stackV: int, d_stackC: int, W: int, H: int, d_out3: int, off_x: int = 0, off_y: int = 0,
                         slot: int = 0):
        """Row f-3 (MatchGPULib.cpp:2589-2701): full-resolution field from the foveated stacks."""
        self.check(self.lib.ugsm_reconstruct_full(self._h, slot, d_stackH, d_stackV, d_stackC, W, H, off_x, off_y, d_out3))
        self.check(self.lib.ugsm_wait(self._h, slot))

    # ---- B pairs per call (ugsm_submit_*_batch): lists of device pointers ---------------------------------------------
    @staticmethod
    def _ptrs(ps):
        return (C.c_void_p * len(ps))(*[int(p) if p is not None else None for p in ps])

    def submit_full_batch(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, d_out):
        n = len(d_rgbL)
        self.check(self.lib.ugsm_submit_full_batch(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, self._ptrs(d_out)))

    def submit_full_checked(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, d_out, d_back, tau: float):
        """Both directions of the pairs in one lockstep call (ugsm_submit_full_checked), each pair's two fields checked against each other at
        threshold tau (> 0; the call's own, not the context's setting).  d_back: None, or one device pointer (or None) per pair for the right
        camera's checked field.  last_lr_marked_pair(slot, k) answers for pair k."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_out) != n or (d_back is not None and len(d_back) != n):
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        self.check(self.lib.ugsm_submit_full_checked(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, self._ptrs(d_out),
                                                     self._ptrs(d_back) if d_back is not None else None, tau))

    def match_full_checked(self, L: np.ndarray, R: np.ndarray, tau: float, back: bool = True):
        """Blocking, from any host memory (ugsm_match_full_checked): the checked (3, H, W) field of the left camera and, with `back`, that of
        the right camera (else None)."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        fwd = np.empty((3, H, W), np.float32)
        bwd = np.empty((3, H, W), np.float32) if back else None
        bp = [bwd[c].ctypes.data for c in range(3)] if back else [None] * 3
        self.check(self.lib.ugsm_match_full_checked(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, *[fwd[c].ctypes.data for c in range(3)], *bp, tau))
        return fwd, bwd

    def last_lr_marked_pair(self, slot: int = 0, pair: int = 0):
        """(forward, backward) pixels the check of the last submit_full_checked / match_full_checked on `slot` marked for pair `pair`."""
        f, b = C.c_longlong(), C.c_longlong()
        self.check(self.lib.ugsm_last_lr_marked_pair(self._h, slot, pair, C.byref(f), C.byref(b)))
        return int(f.value), int(b.value)

    def submit_full_seeded(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, d_prior, start_level: int, d_out):
        """The pairs matched from level start_level downwards, each from its full-resolution prior field (ugsm_submit_full_seeded): lists of
        device pointers, one entry per pair; d_prior[k] may be d_out[k]."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_prior) != n or len(d_out) != n:
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        self.check(self.lib.ugsm_submit_full_seeded(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, self._ptrs(d_prior),
                                                    int(start_level), self._ptrs(d_out)))

    def match_full_seeded(self, L: np.ndarray, R: np.ndarray, prior: np.ndarray, start_level: int) -> np.ndarray:
        """Blocking, from any host memory (ugsm_match_full_seeded): the (3, H, W) field reached from level start_level of `prior` (3, H, W)."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        if tuple(prior.shape) != (3, H, W):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the prior is a (3, H, W) field of the images' size")
        pr = np.ascontiguousarray(prior, np.float32)
        out = np.empty((3, H, W), np.float32)
        self.check(self.lib.ugsm_match_full_seeded(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, *[pr[c].ctypes.data for c in range(3)],
                                                   int(start_level), *[out[c].ctypes.data for c in range(3)]))
        return out

    def stage_restrict(self, d_src3: int, W: int, H: int, level: int, d_dst3: int):
        """The seeded call's restriction alone (ugsm_stage_restrict): level `level`'s starting field from a full-resolution one; waits."""
        self.check(self.lib.ugsm_stage_restrict(self._h, d_src3, W, H, int(level), d_dst3))

    def submit_foveated_warm(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, offsets, d_prior_stack, prior_offsets, start_level: int,
                             d_stack):
        """The pairs matched from fovea level start_level downwards, each from its prior stack matched at prior_offsets[k]
        (ugsm_submit_foveated_warm): lists of device pointers, one entry per pair; offsets: lists of (x, y), None = centred.  Not in place."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_prior_stack) != n or len(d_stack) != n or any(o is not None and len(o) != n for o in (offsets, prior_offsets)):
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        ox, oy = self._offsets(offsets, n)
        px, py = self._offsets(prior_offsets, n)
        self.check(self.lib.ugsm_submit_foveated_warm(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, ox, oy,
                                                      self._ptrs(d_prior_stack), px, py, int(start_level), self._ptrs(d_stack)))

    def submit_foveated_warm_field(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, offsets, d_prior_field, start_level: int, d_stack):
        """The same from full-resolution prior fields, 3 planes of W x H each (ugsm_submit_foveated_warm_field)."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_prior_field) != n or len(d_stack) != n or (offsets is not None and len(offsets) != n):
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        ox, oy = self._offsets(offsets, n)
        self.check(self.lib.ugsm_submit_foveated_warm_field(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, ox, oy,
                                                            self._ptrs(d_prior_field), int(start_level), self._ptrs(d_stack)))

    def match_foveated_warm(self, L: np.ndarray, R: np.ndarray, prior_stack: np.ndarray, prior_off, off, start_level: int) -> np.ndarray:
        """Blocking, from any host memory (ugsm_match_foveated_warm): the (3, F, fovH, fovW) stack of the window at `off` reached from fovea level
        start_level of `prior_stack`, a stack of that shape matched at `prior_off`."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        pr = np.ascontiguousarray(prior_stack, np.float32)
        if pr.ndim != 4 or pr.shape[0] != 3:
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the prior is a (3, F, fovH, fovW) stack")
        out = np.empty(pr.shape, np.float32)
        self.check(self.lib.ugsm_match_foveated_warm(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, int(off[0]), int(off[1]),
                                                     *[pr[c].ctypes.data for c in range(3)], int(prior_off[0]), int(prior_off[1]), int(start_level),
                                                     *[out[c].ctypes.data for c in range(3)]))
        return out

    def stage_warm_stack(self, d_prior_stack: int, W: int, H: int, prior_off, off, start_level: int, d_dst_stack: int):
        """The warm foveated call's starting-field launch alone (ugsm_stage_warm_stack): row blocks start_level .. F-1 of d_dst_stack; waits."""
        self.check(self.lib.ugsm_stage_warm_stack(self._h, d_prior_stack, W, H, int(prior_off[0]), int(prior_off[1]), int(off[0]), int(off[1]),
                                                  int(start_level), d_dst_stack))

    def submit_full_coarse(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, stop_level: int, d_state, d_full=None):
        """The coarse half of a full-mode call (ugsm_submit_full_coarse): the levels top .. stop_level; lists of device pointers, one entry per
        pair.  d_state[k]: level stop_level's field; d_full (None, or a list whose entries may be None): its prolongation to W x H."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_state) != n or (d_full is not None and len(d_full) != n):
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        self.check(self.lib.ugsm_submit_full_coarse(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, int(stop_level),
                                                    self._ptrs(d_state), self._ptrs(d_full) if d_full is not None else None))

    def submit_full_fine(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, d_state, state_level: int, d_out):
        """The fine half (ugsm_submit_full_fine): the levels state_level - 1 .. 0 from the pairs' fields of level state_level."""
        n = len(d_rgbL)
        if len(d_rgbR) != n or len(d_state) != n or len(d_out) != n:
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        self.check(self.lib.ugsm_submit_full_fine(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, self._ptrs(d_state),
                                                  int(state_level), self._ptrs(d_out)))

    def stage_prolong(self, d_src3: int, W: int, H: int, level: int, d_dst3: int):
        """The coarse half's prolongation alone (ugsm_stage_prolong): the W x H field of a field of level `level`; waits."""
        self.check(self.lib.ugsm_stage_prolong(self._h, d_src3, W, H, int(level), d_dst3))

    def match_full_coarse(self, L: np.ndarray, R: np.ndarray, stop_level: int, want_full: bool = False):
        """Blocking, from any host memory (ugsm_match_full_coarse): level stop_level's (3, h, w) field; with want_full, (state, its (3, H, W)
        prolongation)."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        levels = int(self.cfg.levels)
        if not 0 <= int(stop_level) < levels:
            raise UgsmError(UGSM_ERR_BAD_ARG, "stop_level outside 0 .. levels - 1")
        w, h = level_dims(W, H, levels)
        state = np.empty((3, h[stop_level], w[stop_level]), np.float32)
        full = np.empty((3, H, W), np.float32) if want_full else None
        self.check(self.lib.ugsm_match_full_coarse(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, int(stop_level),
                                                   *[state[c].ctypes.data for c in range(3)],
                                                   *[full[c].ctypes.data if want_full else None for c in range(3)]))
        return (state, full) if want_full else state

    def match_full_fine(self, L: np.ndarray, R: np.ndarray, state: np.ndarray, state_level: int) -> np.ndarray:
        """Blocking, from any host memory (ugsm_match_full_fine): the (3, H, W) field reached from `state`, a (3, h, w) field of level state_level."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        levels = int(self.cfg.levels)
        if not 1 <= int(state_level) < levels:
            raise UgsmError(UGSM_ERR_BAD_ARG, "state_level outside 1 .. levels - 1")
        w, h = level_dims(W, H, levels)
        if tuple(state.shape) != (3, h[state_level], w[state_level]):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the state is a (3, h, w) field of level state_level's size")
        st = np.ascontiguousarray(state, np.float32)
        out = np.empty((3, H, W), np.float32)
        self.check(self.lib.ugsm_match_full_fine(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, *[st[c].ctypes.data for c in range(3)],
                                                 int(state_level), *[out[c].ctypes.data for c in range(3)]))
        return out

    def submit_foveated_batch(self, slot: int, d_rgbL, d_rgbR, W: int, H: int, stride: int, offsets, d_stack, d_pyrL=None, d_pyrR=None):
        n = len(d_rgbL)
        ox = (C.c_int * n)(*[int(o[0]) for o in offsets]) if offsets is not None else None
        oy = (C.c_int * n)(*[int(o[1]) for o in offsets]) if offsets is not None else None
        self.check(self.lib.ugsm_submit_foveated_batch(self._h, slot, n, self._ptrs(d_rgbL), self._ptrs(d_rgbR), W, H, stride, ox, oy, self._ptrs(d_stack),
                                                       self._ptrs(d_pyrL) if d_pyrL is not None else None,
                                                       self._ptrs(d_pyrR) if d_pyrR is not None else None))

    def submit_full_batch_host(self, slot: int, rgbL, rgbR, W: int, H: int, stride: int, outs):
        """rgbL / rgbR: lists of page-locked uint8 arrays (host_array); outs: list of page-locked (3, H, W) float32 arrays."""
        n = len(rgbL)
        self.check(self.lib.ugsm_submit_full_batch_host(self._h, slot, n, self._ptrs([a.ctypes.data for a in rgbL]), self._ptrs([a.ctypes.data for a in rgbR]),
                                                        W, H, stride, self._ptrs([o[0].ctypes.data for o in outs]), self._ptrs([o[1].ctypes.data for o in outs]),
                                                        self._ptrs([o[2].ctypes.data for o in outs])))

    def submit_full_checked_host(self, slot: int, rgbL, rgbR, W: int, H: int, stride: int, outs, backs, tau: float):
        """submit_full_checked from page-locked memory (ugsm_submit_full_checked_host).  rgbL / rgbR: lists of page-locked uint8 arrays; outs: list
        of page-locked (3, H, W) float32 arrays for the checked forward fields; backs: None, or a list of such arrays (or None) per pair for the
        right camera's checked fields."""
        n = len(rgbL)
        if len(rgbR) != n or len(outs) != n or (backs is not None and len(backs) != n):
            raise UgsmError(UGSM_ERR_BAD_ARG, "one entry per pair in every list")
        bp = [self._ptrs([b[c].ctypes.data if b is not None else None for b in backs]) if backs is not None else None for c in range(3)]
        self.check(self.lib.ugsm_submit_full_checked_host(self._h, slot, n, self._ptrs([a.ctypes.data for a in rgbL]), self._ptrs([a.ctypes.data for a in rgbR]),
                                                          W, H, stride, *[self._ptrs([o[c].ctypes.data for o in outs]) for c in range(3)], *bp, tau))

    def submit_foveated_batch_host(self, slot: int, rgbL, rgbR, W: int, H: int, stride: int, offsets, stacks):
        """stacks: list of page-locked (3, F, fovH, fovW) float32 arrays."""
        n = len(rgbL)
        ox = (C.c_int * n)(*[int(o[0]) for o in offsets]) if offsets is not None else None
        oy = (C.c_int * n)(*[int(o[1]) for o in offsets]) if offsets is not None else None
        self.check(self.lib.ugsm_submit_foveated_batch_host(self._h, slot, n, self._ptrs([a.ctypes.data for a in rgbL]), self._ptrs([a.ctypes.data for a in rgbR]),
                                                            W, H, stride, ox, oy, self._ptrs([t[0].ctypes.data for t in stacks]),
                                                            self._ptrs([t[1].ctypes.data for t in stacks]), self._ptrs([t[2].ctypes.data for t in stacks])))

    # ---- several fovea windows on ONE pair (ugsm_*_multi): pyramids and the coarse phase once, the windows' fine levels in lockstep -----
    @staticmethod
    def _offsets(offsets, n):
        if offsets is None:
            return None, None
        return (C.c_int * n)(*[int(o[0]) for o in offsets]), (C.c_int * n)(*[int(o[1]) for o in offsets])

    def submit_foveated_multi(self, slot: int, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, offsets, d_stack):
        """d_stack: one device stack per window, each 3 x (F * fovH) x fovW; offsets: one (off_x, off_y) per window, or None (all centred)."""
        n = len(d_stack)
        ox, oy = self._offsets(offsets, n)
        self.check(self.lib.ugsm_submit_foveated_multi(self._h, slot, d_rgbL, d_rgbR, W, H, stride, n, ox, oy, self._ptrs(d_stack)))

    def submit_foveated_multi_checked(self, slot: int, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, offsets, d_stack, tau: float):
        """submit_foveated_multi with the foveated LR check at threshold tau (> 0; the call's own, not the context's setting): both directions
        in lockstep, stackC zeroed where the match does not point back.  last_lr_marked_levels(slot, k) answers for window k."""
        n = len(d_stack)
        ox, oy = self._offsets(offsets, n)
        self.check(self.lib.ugsm_submit_foveated_multi_checked(self._h, slot, d_rgbL, d_rgbR, W, H, stride, n, ox, oy, self._ptrs(d_stack), tau))

    def match_foveated_multi(self, L: np.ndarray, R: np.ndarray, offsets, tau=None):
        """Blocking, from any host memory: the (3, F, fovH, fovW) stacks of the windows at `offsets`, one array per window.  tau (> 0): the
        checked call (ugsm_match_foveated_multi_checked)."""
        W, H, stride = self.check_image(L)
        if self.check_image(R) != (W, H, stride):
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "the two images differ in size or stride")
        n = len(offsets)
        if n < 1:
            raise UgsmError(UGSM_ERR_BAD_ARG, "no window")
        fw, fh = fovea_dims(W, H, self.cfg.levels, self.cfg.fovea_levels)
        stacks = [np.empty((3, self.cfg.fovea_levels, fh, fw), np.float32) for _ in range(n)]
        ox, oy = self._offsets(offsets, n)
        planes = [self._ptrs([t[c].ctypes.data for t in stacks]) for c in range(3)]
        if tau is None:
            self.check(self.lib.ugsm_match_foveated_multi(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, n, ox, oy, *planes))
        else:
            self.check(self.lib.ugsm_match_foveated_multi_checked(self._h, L.ctypes.data, R.ctypes.data, W, H, stride, n, ox, oy, *planes, tau))
        return stacks

    def match_foveated_multi_checked(self, L: np.ndarray, R: np.ndarray, offsets, tau: float):
        return self.match_foveated_multi(L, R, offsets, tau)

    def reconstruct_full_multi(self, d_stack, W: int, H: int, d_out3: int, offsets=None, slot: int = 0):
        """Row f-3 over the stacks of several windows of one pair: where windows overlap the highest index wins.  Waits."""
        n = len(d_stack)
        ox, oy = self._offsets(offsets, n)
        self.check(self.lib.ugsm_reconstruct_full_multi(self._h, slot, n, self._ptrs(d_stack), W, H, ox, oy, d_out3))
        self.check(self.lib.ugsm_wait(self._h, slot))

    # ---- the queue (ugsm_enqueue_* / ugsm_flush / ugsm_next_done): the library owns the slots ----------------------------------------
    def enqueue_full(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, d_out: int, tag: int):
        self.check(self.lib.ugsm_enqueue_full(self._h, d_rgbL, d_rgbR, W, H, stride, d_out, tag))

    def enqueue_foveated(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, off, d_stack: int, tag: int, d_pyrL=None, d_pyrR=None):
        self.check(self.lib.ugsm_enqueue_foveated(self._h, d_rgbL, d_rgbR, W, H, stride, int(off[0]), int(off[1]), d_stack, d_pyrL, d_pyrR, tag))

    def enqueue_full_host(self, rgbL: np.ndarray, rgbR: np.ndarray, out3: np.ndarray, tag: int):
        """rgbL / rgbR: page-locked (H, W, 3) uint8 (host_array; (H, W) or (H, W, 4) in other input formats); out3: page-locked (3, H, W) float32."""
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_full_host(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, out3[0].ctypes.data,
                                                   out3[1].ctypes.data, out3[2].ctypes.data, tag))

    def enqueue_foveated_host(self, rgbL: np.ndarray, rgbR: np.ndarray, off, stack3: np.ndarray, tag: int, pyrL=None, pyrR=None):
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_foveated_host(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, int(off[0]), int(off[1]),
                                                       stack3[0].ctypes.data, stack3[1].ctypes.data, stack3[2].ctypes.data,
                                                       pyrL.ctypes.data if pyrL is not None else None, pyrR.ctypes.data if pyrR is not None else None, tag))

    def enqueue_full_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, tag: int):
        """Any host memory: the images are copied before the call returns; the results come back in ugsm_completion.result."""
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_full_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, tag))

    def enqueue_foveated_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, off, want_pyramids: bool, tag: int):
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_foveated_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, int(off[0]), int(off[1]),
                                                          1 if want_pyramids else 0, tag))

    # ... with the pair's cloud (ugsm_enqueue_*_cloud*): spec is a QueueCloud (queue_cloud())
    def enqueue_full_cloud(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, d_out: int, spec: QueueCloud, d_points: int, cap_points: int,
                           d_count: int, tag: int):
        self.check(self.lib.ugsm_enqueue_full_cloud(self._h, d_rgbL, d_rgbR, W, H, stride, d_out, C.byref(spec), d_points, int(cap_points), d_count, tag))

    def enqueue_foveated_cloud(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, off, d_stack: int, spec: QueueCloud, d_points: int,
                               cap_points: int, d_count: int, tag: int, d_level_counts=None):
        self.check(self.lib.ugsm_enqueue_foveated_cloud(self._h, d_rgbL, d_rgbR, W, H, stride, int(off[0]), int(off[1]), d_stack, C.byref(spec), d_points,
                                                        int(cap_points), d_count, d_level_counts, tag))

    def enqueue_full_cloud_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, spec: QueueCloud, tag: int):
        """Any host memory in; the cloud comes back through done_cloud() after the next_done() that reports the pair."""
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_full_cloud_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, C.byref(spec), tag))

    def enqueue_foveated_cloud_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, off, spec: QueueCloud, tag: int):
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_foveated_cloud_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, int(off[0]), int(off[1]),
                                                                C.byref(spec), tag))

    # ... checked (ugsm_enqueue_full_checked*): both directions of a call's pairs in lockstep, each pair with its own tau (> 0), whatever
    # set_lr_check holds; d_back: the right camera's checked field, or None
    def enqueue_full_checked(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, d_out: int, d_back, tau: float, tag: int):
        self.check(self.lib.ugsm_enqueue_full_checked(self._h, d_rgbL, d_rgbR, W, H, stride, d_out, d_back, tau, tag))

    def enqueue_full_checked_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, tau: float, want_back: bool, tag: int):
        """Any host memory in; the checked forward planes come back in ugsm_completion.result[0..2], the right camera's (want_back) through
        done_checked()."""
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_full_checked_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, tau, 1 if want_back else 0, tag))

    def enqueue_full_checked_cloud(self, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, d_out: int, d_back, tau: float, spec: QueueCloud,
                                   d_points: int, cap_points: int, d_count: int, tag: int):
        self.check(self.lib.ugsm_enqueue_full_checked_cloud(self._h, d_rgbL, d_rgbR, W, H, stride, d_out, d_back, tau, C.byref(spec), d_points,
                                                            int(cap_points), d_count, tag))

    def enqueue_full_checked_cloud_managed(self, rgbL: np.ndarray, rgbR: np.ndarray, tau: float, want_back: bool, spec: QueueCloud, tag: int):
        W, H, stride = self._pair(rgbL, rgbR)
        self.check(self.lib.ugsm_enqueue_full_checked_cloud_managed(self._h, rgbL.ctypes.data, rgbR.ctypes.data, W, H, stride, tau,
                                                                    1 if want_back else 0, C.byref(spec), tag))

    def done_checked(self, shape=None):
        """For the checked pair the last next_done() reported: (marked_fwd, marked_back, back).  back: None, or -- a managed pair enqueued with
        want_back, `shape` = (H, W) given -- a (3, H, W) copy of the right camera's checked planes (the library's page-locked staging itself is
        lent only until the next next_done() on the context)."""
        r = CheckedResult()
        self.check(self.lib.ugsm_done_checked(self._h, C.byref(r)))
        back = None
        if shape is not None and r.back[0]:
            H, W = shape
            back = np.stack([np.ctypeslib.as_array(r.back[c], shape=(H, W)) for c in range(3)])
        return int(r.marked_fwd), int(r.marked_back), back

    def done_cloud(self):
        """The managed cloud of the pair the last next_done() reported: (records, count, level_counts).  records is a numpy view of the library's
        page-locked staging (CLOUD_PCL32 or CLOUD_XYZRGB16, `stored` of them), valid until the next next_done() on the context: copy what is to be kept."""
        r = CloudResult()
        self.check(self.lib.ugsm_done_cloud(self._h, C.byref(r)))
        dt = CLOUD_PCL32 if r.point_step == 32 else CLOUD_XYZRGB16
        if r.stored > 0:
            buf = (C.c_char * (int(r.stored) * r.point_step)).from_address(r.points)
            rec = np.frombuffer(buf, dtype=dt)
        else:
            rec = np.empty(0, dt)
        return rec, int(r.count), [int(r.level_counts[k]) for k in range(r.levels)]

    def _pair(self, rgbL: np.ndarray, rgbR: np.ndarray):
        g = self.check_image(rgbL)
        if self.check_image(rgbR) != g:
            raise UgsmError(UGSM_ERR_SIZE_MISMATCH, "left and right images differ in size or stride")
        return g

    def flush(self):
        self.check(self.lib.ugsm_flush(self._h))

    def next_done(self, block: bool = True):
        """The oldest pair not yet reported as a Completion, or None (block=False: not finished yet, or nothing outstanding; block=True:
        nothing outstanding).  A completion whose call failed raises UgsmError with `.tag` set: the pair has been reported -- the library will not
        name it again -- so whoever keeps per-tag state drops it before handling the error."""
        c = Completion()
        st = self.lib.ugsm_next_done(self._h, C.byref(c), 1 if block else 0)
        if st in (UGSM_PENDING, UGSM_EMPTY):
            return None
        self.check(st)
        if c.status:
            raise UgsmError(c.status, f"pair {c.tag}: {status_string(c.status)}: {self.lib.ugsm_last_error(self._h).decode()}", tag=int(c.tag))
        return c

    def drain(self):
        """Flushes and fetches every outstanding completion, oldest first."""
        out = []
        while True:
            c = self.next_done(True)
            if c is None:
                return out
            out.append(c)

    def queue_depth(self):
        w, f, u = C.c_int(), C.c_int(), C.c_int()
        self.check(self.lib.ugsm_queue_depth(self._h, C.byref(w), C.byref(f), C.byref(u)))
        return w.value, f.value, u.value

    @staticmethod
    def managed_planes(c: "Completion", shapes):
        """numpy views (valid until the next next_done on the context) of a managed completion's result planes; shapes: one per plane wanted."""
        out = []
        for k, shp in enumerate(shapes):
            n = int(np.prod(shp))
            out.append(np.ctypeslib.as_array(c.result[k], shape=(n,)).reshape(shp))
        return out

    # ---- the fovea shard with RCCL inside the library (ugsm_shard_*) ------------------------------------------------------------------
    def shard_init(self, id128: bytes, rank: int, world: int):
        buf = (C.c_char * UGSM_SHARD_ID_BYTES).from_buffer_copy(id128)
        self.check(self.lib.ugsm_shard_init(self._h, buf, rank, world))

    def shard_count_ranks(self) -> int:
        n = C.c_int()
        self.check(self.lib.ugsm_shard_count_ranks(self._h, C.byref(n)))
        return n.value

    def submit_fovea_shard(self, slot: int, d_rgbL: int, d_rgbR: int, W: int, H: int, stride: int, off, d_stack: int, src_rank: int = 0):
        self.check(self.lib.ugsm_submit_fovea_shard(self._h, slot, d_rgbL, d_rgbR, W, H, stride, int(off[0]), int(off[1]), d_stack, src_rank))

    def shard_set_timeout(self, milliseconds: int):
        self.check(self.lib.ugsm_shard_set_timeout(self._h, int(milliseconds)))

    def shard_init_all(self, others=()):
        """One process, several GPUs: this context and `others` (each on its own device) become ranks 0 .. n-1 of one communicator."""
        hs = (C.c_void_p * (1 + len(others)))(self._h, *[o._h for o in others])
        self.check(self.lib.ugsm_shard_init_all(hs, 1 + len(others)))

    def shard_gather(self, slot: int, d_stack: int, stack_floats: int, d_all, dst_rank: int = 0):
        self.check(self.lib.ugsm_shard_gather(self._h, slot, d_stack, stack_floats, d_all, dst_rank))

    def shard_finalize(self):
        self.check(self.lib.ugsm_shard_finalize(self._h))

    def range_words(self, slot: int, n: int = 1):
        """libugsm_dev.so only (include/ugsm_dev.h): the range words of the n pairs of the slot's last call, read after the slot has drained --
        1 where a pyramid value of the pair was outside range_ok (csrc/ugsm_exact.hpp) and K-cost took the compiler's division."""
        out = (C.c_uint * n)()
        self.check(self.lib.ugsm_stage_range_words(self._h, slot, out, n))
        return [int(v) for v in out]

    def device_bytes(self) -> int:
        return int(self.lib.ugsm_context_device_bytes(self._h))

    def kernel_stats(self):
        """One dict per (kernel, pyramid level) with harvested launches; level -1 = not tied to a level."""
        cap = 512
        arr = (KernelStat * cap)()
        n = self.lib.ugsm_get_kernel_stats(self._h, arr, cap)
        return [dict(name=arr[k].name.decode(), level=int(arr[k].level), launches=int(arr[k].launches), total_ms=float(arr[k].total_ms),
                     pixel_launches=float(arr[k].pixel_launches)) for k in range(min(n, cap))]

    def set_profile_events(self, mode: int):
        self.check(self.lib.ugsm_set_profile_events(self._h, int(mode)))

    def reset_kernel_stats(self):
        self.check(self.lib.ugsm_reset_kernel_stats(self._h))


def plan_level(W: int, H: int, alone: bool = True, **cfg_fields):
    """Which kernels a W x H level runs (host only): dict of ugsm_level_plan; cfg_fields override the default ugsm_config.
    alone: the call has the chip to itself (what the library decides per call from what is in flight; include/ugsm.h)."""
    lib = load(bool(cfg_fields.get("kernel_path") == 1 or cfg_fields.get("march_min_pixels", 0) < 0 or cfg_fields.pop("dev", False)))
    cfg = Config()
    lib.ugsm_default_config(C.byref(cfg))
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    out = LevelPlan()
    st = lib.ugsm_plan_level(C.byref(cfg), 1 if alone else 0, W, H, C.byref(out))
    if st != 0:
        raise UgsmError(st, "ugsm_plan_level")
    return {k: int(getattr(out, k)) for k in ("cost_kernel", "smooth_kernel", "smooth_rh", "strip_rows", "seed_fused", "smooth_tile_rows", "alone", "pairs_per_launch")}


def shard_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 makes one and hands it to the other ranks out of band)."""
    buf = (C.c_char * UGSM_SHARD_ID_BYTES)()
    st = load().ugsm_shard_unique_id(buf)
    if st != 0:
        raise UgsmError(st, "ugsm_shard_unique_id: " + status_string(st))
    return bytes(buf)


def queue_plan(n_pairs: int, **cfg_fields):
    """The calls the queue forms from a burst of n_pairs pairs enqueued from idle and flushed (host only)."""
    lib = load()
    cfg = Config()
    lib.ugsm_default_config(C.byref(cfg))
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    cap = max(1, n_pairs)
    sizes = (C.c_int * cap)()
    n = lib.ugsm_queue_plan(C.byref(cfg), n_pairs, sizes, cap)
    if n < 0:
        raise UgsmError(UGSM_ERR_BAD_ARG, "ugsm_queue_plan")
    return list(sizes[:n])


def fovea_mapping(W: int, H: int, src_level: int, dest_level: int = 0):
    """getPointCloud.cpp:387-484 -> (left_margin, upper_margin, scale); host only."""
    lib = load()
    l, u, sc = C.c_int(), C.c_int(), C.c_float()
    st = lib.ugsm_fovea_mapping(W, H, src_level, dest_level, C.byref(l), C.byref(u), C.byref(sc))
    if st != 0:
        raise UgsmError(st, "ugsm_fovea_mapping")
    return l.value, u.value, np.float32(sc.value)
