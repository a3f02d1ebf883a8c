"""Host-side mirror of the reference's `MatchGPULib` class over the C-ABI.

Same method names, argument meaning and results as
/root/reference/src/gpu_matcher/MatchGPULib.h:6-47, so call sites written against the
reference (UG_GPU_matcher.cpp:160-181,423,530-535,645) read the same.  Images are numpy
`uint8` arrays of shape (rows, cols, 3) in rgb8 order -- what `cv_bridge::toCvCopy(msg,
RGB8)->image` holds -- or `float32` arrays, (rows, cols, 3) or (rows, cols), which the library
reads as they stand (UGSM_INPUT_RGB32F / UGSM_INPUT_MONO32F: a 32FC3 / 32FC1 image, a 16-bit
camera's v / 256).  Differences, all deliberate:
  * results are returned as numpy arrays owned by the caller (the reference mallocs and
    expects the caller to free, UG_GPU_matcher.cpp:487-489);
  * one persistent context per object, no cudaDeviceReset per call (MatchGPULib.cpp:400);
  * a failed call raises UgsmError instead of exit(EXIT_FAILURE).
The C++ twin of this class for the ROS node is ros/MatchGPULib_ugsm.hpp.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, UgsmError


def _parse_argv(argv):
    """findCudaDevice's -device=N (MatchGPULib.cpp:254) and argv[2] = fovea levels (:259-264)."""
    device, fovea_levels = 0, 7
    argv = list(argv or [])
    for a in argv:
        if isinstance(a, str) and a.startswith("-device="):
            device = int(a.split("=", 1)[1])
    if len(argv) > 2:
        try:
            fovea_levels = int(argv[2])
        except ValueError:
            fovea_levels = 0  # atoi() of a non-number
    return device, fovea_levels


def _as_image(img):
    """(array, UGSM_INPUT_*): a uint8 (rows, cols, 3) rgb8 image, or a float32 image read as it stands -- (rows, cols, 3) as rgb32f,
    (rows, cols) as mono32f (level 0 of the pyramid is these floats; samples finite and >= 0).  Rows may be padded, pixels are contiguous."""
    a = np.asarray(img)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        fmt, pixel = _lib.UGSM_INPUT_RGB8, (3, 1)
    elif a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 3:
        fmt, pixel = _lib.UGSM_INPUT_RGB32F, (12, 4)
    elif a.dtype == np.float32 and a.ndim == 2:
        fmt, pixel = _lib.UGSM_INPUT_MONO32F, (4,)
    else:
        raise UgsmError(_lib.UGSM_ERR_BAD_ARG, "image must be uint8 (rows, cols, 3) rgb8, or float32 (rows, cols, 3) / (rows, cols)")
    if a.strides[1:] != pixel or a.strides[0] % a.itemsize:
        a = np.ascontiguousarray(a)
    return a, fmt


class MatchGPULib:
    MAX_LEVEL = 14  # MatchLib_common.h:13
    float_images = True  # float32 images are read as they stand (_as_image): the service hands 32FC3 / 32FC1 payloads over in place

    def __init__(self, argc: int = 0, argv=None, *, levels: int = MAX_LEVEL, kernel_path: int = 0, frames_in_flight: int = 1):
        """frames_in_flight > 1 (not in the reference): the context gets min(frames_in_flight, 4) slots and the pipelined calls below
        (enqueueMatch / enqueueStack / nextDone) keep that many pairs outstanding in the library's queue; the blocking calls are unchanged."""
        device, fl = _parse_argv(argv if argc else None)
        self.foveatedmatching = 0
        self.foveatelevel = fl
        self.fovH = 0
        self.fovW = 0
        self._levels = levels
        self.frames_in_flight = max(1, int(frames_in_flight))
        slots = min(self.frames_in_flight, 4)
        batch = min(8, -(-self.frames_in_flight // slots))
        self._ctx = Context(device=device, levels=levels, fovea_levels=fl, slots=slots, kernel_path=kernel_path, batch=batch)
        self._tags = {}     # tag -> (kind, rows, cols, want_pyr) of the pairs outstanding in the queue

    def _take(self, cv_ptrL, cv_ptrR):
        """The pair as the library reads it, in place, and the context's input format set to match (ugsm_set_input_format: captured by the
        call that follows)."""
        (L, fl), (R, fr) = _as_image(cv_ptrL), _as_image(cv_ptrR)
        if fl != fr or L.shape != R.shape or L.strides[0] != R.strides[0]:
            raise UgsmError(_lib.UGSM_ERR_SIZE_MISMATCH, "left/right images differ in size or format")
        if self._ctx.input_format != fl:
            self._ctx.set_input_format(fl)
        return L, R

    # -- getters / setters, MatchGPULib.cpp:268-301 --
    def getFoveaWidth(self) -> int:
        return self.fovW

    def getFoveaHeight(self) -> int:
        return self.fovH

    def getFoveateLevel(self) -> int:
        return self.foveatelevel

    def setFoveaWidth(self, rows: int):
        self.fovW = rows

    def setFoveaHeight(self, cols: int):
        self.fovH = cols

    def setFoveated(self, fov: int):
        self.foveatedmatching = fov

    # -- initStack, MatchGPULib.cpp:406-426 --
    def initStack(self, cv_ptrL, cv_ptrR=None) -> int:
        rows, cols = np.asarray(cv_ptrL).shape[:2]
        fw, fh = _lib.fovea_dims(cols, rows, self._levels, self.foveatelevel)
        self.setFoveaHeight(fh)
        self.setFoveaWidth(fw)
        return 0

    # -- match, MatchGPULib.cpp:303-403 --
    def match(self, cv_ptrL, cv_ptrR, fov: int = 0, tau=None):
        """Returns finDisp: float32 (3, rows, cols) = horizontal, vertical disparity and confidence.
        tau (> 0, fov == 0; not in the reference): the LR check for this call alone, both directions in one lockstep call
        (ugsm_match_full_checked) -- returns (finDisp, backDisp): the checked fields of the left and of the right camera."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = fov
        if tau is not None:
            if fov != 0:
                raise UgsmError(_lib.UGSM_ERR_BAD_ARG, "match(.., tau) is the full-mode call: fov must be 0")
            return self._ctx.match_full_checked(L, R, tau)
        rows, cols = L.shape[:2]
        out = np.empty((3, rows, cols), np.float32)
        c = self._ctx
        if fov == 1:
            # foveated matching + hierarchicalDisparity (MatchGPULib.cpp:354-360); the node never asks for it
            # (UG_GPU_matcher.cpp:421-423,644-645), SURVEY 8f row f-3
            self.fovW, self.fovH = _lib.fovea_dims(cols, rows, self._levels, self.foveatelevel)
            c.check(c.lib.ugsm_match_foveated_full(c.handle, L.ctypes.data, R.ctypes.data, cols, rows, L.strides[0], 0, 0,
                                                   out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
            return out
        c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, cols, rows, L.strides[0],
                                      out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return out

    def matchSeeded(self, cv_ptrL, cv_ptrR, prior, start_level: int) -> np.ndarray:
        """(not in the reference) match(L, R, 0) started at level start_level from `prior`, a finDisp of the images' size -- the previous
        frame's, say -- instead of from the zero seed at the top level (ugsm_match_full_seeded).  Returns finDisp."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = 0
        return self._ctx.match_full_seeded(L, R, np.asarray(prior, np.float32), start_level)

    def matchCoarse(self, cv_ptrL, cv_ptrR, stop_level: int, want_full: bool = False):
        """(not in the reference) match(L, R, 0) stopped when level stop_level has finished (ugsm_match_full_coarse): that level's field,
        (3, h, w) of the level's size; with want_full, (state, its prolongation to the images' size, a finDisp)."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = 0
        return self._ctx.match_full_coarse(L, R, stop_level, want_full)

    def matchFine(self, cv_ptrL, cv_ptrR, state, state_level: int) -> np.ndarray:
        """(not in the reference) the rest of match(L, R, 0) from `state`, the field of level state_level that matchCoarse returned
        (ugsm_match_full_fine): with the same pair, match(L, R, 0)'s finDisp bit for bit.  Returns finDisp."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = 0
        return self._ctx.match_full_fine(L, R, np.asarray(state, np.float32), state_level)

    # -- hierarchicalDisparity, MatchGPULib.cpp:2589-2701 --
    def hierarchicalDisparity(self, foveated: np.ndarray, widthInit: int, heightInit: int) -> np.ndarray:
        """foveated: (foveatelevel, 3, fovH, fovW) as matchStack returns it -> (3, heightInit, widthInit)."""
        st = np.ascontiguousarray(np.transpose(np.asarray(foveated, np.float32), (1, 0, 2, 3)))
        c = self._ctx
        ps = [c.to_device(st[k]) for k in range(3)]
        pout = c.alloc(3 * widthInit * heightInit * 4)
        try:
            c.reconstruct_full(ps[0], ps[1], ps[2], widthInit, heightInit, pout)
            return c.to_host(pout, (3, heightInit, widthInit))
        finally:
            for p in ps + [pout]:
                c.free(p)

    # -- the depth image (not in the reference's library: its point-cloud node builds range_map on the host) --
    def depthImage(self, cv_ptrL, cv_ptrR, P1, P2, encoding: str = "32FC1", unit: float = 1.0, min_conf: float = float("-inf"),
                   z_min: float = float("-inf"), z_max: float = float("inf"), factor: float = 1.0, planes: bool = False):
        """match(L, R, 0) and its REP 118 depth image registered to the left camera (ugsm_match_full_depth): "32FC1" -- float32 metres, NaN
        where there is no reading -- or "16UC1" -- uint16 millimetres, 0 where there is none; unit = metres per unit of the calibration.
        Returns the (dh, dw) image; with planes, (image, finDisp) -- otherwise only the image crosses the bus."""
        if encoding not in _lib.DEPTH_ENCODINGS:
            raise UgsmError(_lib.UGSM_ERR_BAD_ARG, f"depth encoding {encoding!r}: 32FC1 or 16UC1")
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = 0
        prm = _lib.depth_params(format=_lib.DEPTH_ENCODINGS[encoding], unit=unit, min_conf=min_conf, z_min=z_min, z_max=z_max, factor=factor)
        return self._ctx.match_full_depth(L, R, P1, P2, prm, planes=planes)

    def depthImageFrame(self, cv_ptrL, cv_ptrR, P1, P2, encoding: str = "32FC1", unit: float = 1.0, min_conf: float = float("-inf"),
                        z_min: float = float("-inf"), z_max: float = float("inf"), factor: float = 1.0, off_x: int = 0, off_y: int = 0,
                        stack: bool = False):
        """The foveated match of (L, R) at window offset (off_x, off_y) and the REP 118 depth image of the WHOLE frame from its stack
        (ugsm_match_foveated_depth): what hierarchicalDisparity of matchStack's result followed by the depth image of that field gives, without
        the field.  Encodings and unit as depthImage.  Returns the (dh, dw) image; with stack, (image, stack as matchStack returns it)."""
        if encoding not in _lib.DEPTH_ENCODINGS:
            raise UgsmError(_lib.UGSM_ERR_BAD_ARG, f"depth encoding {encoding!r}: 32FC1 or 16UC1")
        L, R = self._take(cv_ptrL, cv_ptrR)
        self.foveatedmatching = 1
        prm = _lib.depth_params(format=_lib.DEPTH_ENCODINGS[encoding], unit=unit, min_conf=min_conf, z_min=z_min, z_max=z_max, factor=factor)
        if not stack:
            return self._ctx.match_foveated_depth(L, R, P1, P2, prm, off=(off_x, off_y))
        img, st = self._ctx.match_foveated_depth(L, R, P1, P2, prm, off=(off_x, off_y), stack=True)
        return img, np.ascontiguousarray(np.transpose(st, (1, 0, 2, 3)))

    # -- lens distortion (not in the reference: its cloud node reads K and D and never uses them) --
    def setLens(self, K1, D1, K2, D2, iterations: int = 5):
        """The plumb_bob K and D of the two CameraInfo messages: depthImage and every cloud taken from this matcher's context undistort the two
        pixel positions of each correspondence before they triangulate (ugsm_set_lens)."""
        self._ctx.set_lens(K1, D1, K2, D2, iterations)

    def clearLens(self):
        self._ctx.clear_lens()

    # -- warpRightImage, MatchGPULib.cpp:1445-1518 --
    def warpRightImage(self, right, disparity, channels: int, imageW: int, imageH: int) -> np.ndarray:
        """right: `channels` float planes of imageH x imageW; disparity[0] / disparity[1]: the horizontal / vertical field.  Returns the
        warped planes, float32 (channels, imageH, imageW): out[j][y][x] = right[j] at the texel the matcher fetches for (x, y)."""
        src = np.ascontiguousarray(np.asarray(right, np.float32)[:channels]).reshape(channels, imageH, imageW)
        dx = np.ascontiguousarray(np.asarray(disparity[0], np.float32)).reshape(imageH, imageW)
        dy = np.ascontiguousarray(np.asarray(disparity[1], np.float32)).reshape(imageH, imageW)
        c = self._ctx
        ps = [c.to_device(src), c.to_device(dx), c.to_device(dy), c.alloc(src.nbytes)]
        try:
            c.warp_planes(ps[0], channels, imageW, imageH, ps[1], ps[2], ps[3])
            return c.to_host(ps[3], (channels, imageH, imageW))
        finally:
            for p in ps:
                c.free(p)

    def _stack(self, cv_ptrL, cv_ptrR, want_pyr: bool, off_x: int = 0, off_y: int = 0):
        L, R = self._take(cv_ptrL, cv_ptrR)
        rows, cols = L.shape[:2]
        F = self.foveatelevel
        fw, fh = _lib.fovea_dims(cols, rows, self._levels, F)
        self.fovW, self.fovH = fw, fh  # matching() sets them too, MatchGPULib.cpp:1233-1234
        stack = np.empty((3, F, fh, fw), np.float32)
        pl = np.empty((F, 3, fh, fw), np.float32) if want_pyr else None
        pr = np.empty((F, 3, fh, fw), np.float32) if want_pyr else None
        c = self._ctx
        c.check(c.lib.ugsm_match_foveated(c.handle, L.ctypes.data, R.ctypes.data, cols, rows, L.strides[0], off_x, off_y,
                                          stack[0].ctypes.data, stack[1].ctypes.data, stack[2].ctypes.data,
                                          pl.ctypes.data if want_pyr else None, pr.ctypes.data if want_pyr else None))
        # reference indexing is disparity[level][plane][row*fovW + col]
        return np.ascontiguousarray(stack.transpose(1, 0, 2, 3)), pl, pr

    # -- matchStack, MatchGPULib.cpp:429-531 --
    def matchStack(self, cv_ptrL, cv_ptrR, off_x: int = 0, off_y: int = 0) -> np.ndarray:
        """Returns float32 (foveatelevel, 3, fovH, fovW): [level][dx|dy|conf]."""
        return self._stack(cv_ptrL, cv_ptrR, False, off_x, off_y)[0]

    def matchStackSeeded(self, cv_ptrL, cv_ptrR, prior_stack, prior_off, off, start_level: int) -> np.ndarray:
        """(not in the reference) matchStack(L, R, *off) started at fovea level start_level from `prior_stack` -- what matchStack returned for
        the previous frame at the offsets `prior_off`, which may differ from `off` -- instead of from the zero seed at the top level
        (ugsm_match_foveated_warm).  Returns float32 (foveatelevel, 3, fovH, fovW); the levels above start_level are the prior carried over."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        rows, cols = L.shape[:2]
        F = self.foveatelevel
        fw, fh = _lib.fovea_dims(cols, rows, self._levels, F)
        prior = np.asarray(prior_stack, np.float32)
        if prior.shape != (F, 3, fh, fw):
            raise UgsmError(_lib.UGSM_ERR_SIZE_MISMATCH, "the prior is a stack as matchStack returns it: (foveatelevel, 3, fovH, fovW)")
        self.fovW, self.fovH = fw, fh
        stack = self._ctx.match_foveated_warm(L, R, np.ascontiguousarray(prior.transpose(1, 0, 2, 3)), prior_off, off, start_level)
        return np.ascontiguousarray(stack.transpose(1, 0, 2, 3))

    # -- several windows of one pair (not in the reference; include/ugsm.h, "several fovea windows on ONE pair") --
    def matchStackMulti(self, cv_ptrL, cv_ptrR, offsets, tau=None):
        """matchStack for every (off_x, off_y) of `offsets` (1 .. 16) in one call -- pyramids and the coarse levels once, the windows' fine
        levels in lockstep.  Returns one float32 (foveatelevel, 3, fovH, fovW) per window, each what matchStack returns for its offset.
        tau (> 0): the checked call -- both directions in lockstep, each stack what matchStack returns under setLRCheck(tau, 2)."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        rows, cols = L.shape[:2]
        self.fovW, self.fovH = _lib.fovea_dims(cols, rows, self._levels, self.foveatelevel)
        stacks = self._ctx.match_foveated_multi(L, R, [(int(x), int(y)) for x, y in offsets], tau)
        return [np.ascontiguousarray(st.transpose(1, 0, 2, 3)) for st in stacks]

    # -- matchStackPyramid, MatchGPULib.cpp:534-700 --
    def matchStackPyramid(self, cv_ptrL, cv_ptrR, off_x: int = 0, off_y: int = 0):
        """Returns (disparity stack, leftFov, rightFov); the latter two are (foveatelevel, 3, fovH, fovW)."""
        return self._stack(cv_ptrL, cv_ptrR, True, off_x, off_y)

    # -- the pipelined twin of match / matchStack / matchStackPyramid (not in the reference; include/ugsm.h "the queue") --
    def enqueueMatch(self, cv_ptrL, cv_ptrR, tag: int):
        """match(L, R, 0) without the wait: the images are copied before the call returns; the result comes out of nextDone."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self._ctx.enqueue_full_managed(L, R, tag)
        self._tags[tag] = ("full", L.shape[0], L.shape[1], False)
        self._ctx.flush()   # a frame that arrives starts at once if a slot is free; under load the backlog batches itself

    def enqueueMatchChecked(self, cv_ptrL, cv_ptrR, tau: float, tag: int):
        """enqueueMatch with the LR check of this pair at threshold tau (> 0; ugsm_enqueue_full_checked_managed): both directions of the pairs of a
        call in lockstep, whatever the context's own setting; nextDone hands out the checked field of the left camera."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        self._ctx.enqueue_full_checked_managed(L, R, float(tau), False, tag)
        self._tags[tag] = ("full", L.shape[0], L.shape[1], False)
        self._ctx.flush()

    def enqueueStack(self, cv_ptrL, cv_ptrR, tag: int, want_pyr: bool = False, off_x: int = 0, off_y: int = 0):
        """matchStack / matchStackPyramid without the wait."""
        L, R = self._take(cv_ptrL, cv_ptrR)
        rows, cols = L.shape[:2]
        self.fovW, self.fovH = _lib.fovea_dims(cols, rows, self._levels, self.foveatelevel)
        self._ctx.enqueue_foveated_managed(L, R, (off_x, off_y), want_pyr, tag)
        self._tags[tag] = ("stack", rows, cols, bool(want_pyr))
        self._ctx.flush()

    def outstanding(self) -> int:
        return len(self._tags)

    def nextDone(self, block: bool = True):
        """The oldest outstanding pair: (tag, result) with result as match / matchStack / matchStackPyramid return it (copies owned by the
        caller), or None if there is none (block=False: or it has not finished).  A pair whose call failed raises UgsmError (`.tag` names it);
        it no longer counts as outstanding."""
        try:
            c = self._ctx.next_done(block)
        except UgsmError as e:
            if e.tag is not None:
                self._tags.pop(e.tag, None)
            raise
        if c is None:
            return None
        kind, rows, cols, want_pyr = self._tags.pop(c.tag)
        if kind == "full":
            h, v, cf = self._ctx.managed_planes(c, [(rows, cols)] * 3)
            return c.tag, np.stack([h, v, cf])
        F = self.foveatelevel
        fw, fh = _lib.fovea_dims(cols, rows, self._levels, F)
        shapes = [(F, fh, fw)] * 3 + ([(F, 3, fh, fw)] * 2 if want_pyr else [])
        pl = self._ctx.managed_planes(c, shapes)
        stack = np.ascontiguousarray(np.stack(pl[:3]).transpose(1, 0, 2, 3))   # [level][plane][row][col], as matchStack
        if want_pyr:
            return c.tag, (stack, pl[3].copy(), pl[4].copy())
        return c.tag, stack

    def close(self):
        self._ctx.close()
