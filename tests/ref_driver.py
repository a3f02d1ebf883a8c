"""Runs the reference's host driver (MatchGPULib.cpp compiled for the CPU behind oracle/ref_cpu/ref_driver.cpp: oracle/_ref/ref_driver) as a
child process, and names the cases of the fixtures it wrote -- test infrastructure, shared by tests/golden/make_driver_golden.py,
tests/test_ref_driver_host.py and tests/test_gpu_ref_driver.py.

The cases run the class's own constants: MAX_LEVEL 14 and foveatelevel 7 (levels=14, fovea_levels=7 on this project's side).

  A  231 x 211  synth pair.  211 is the smallest odd size that ugsm_level_dims(W, H, 14) accepts (209 ends below one pixel); 231 is the
                smallest odd width above it whose level sizes differ from the height's at every level down to 4 x 3 (213 .. 229 share the
                coarse levels with 211), so that no exchange of width and height anywhere in the schedule can go unseen.
  B  333 x 251  synth pair, ragged at every level.
  C  231 x 211  the half-black pair of tests/dark_np.py (dark_pair of A's pair): 0 / 0 = NaN in the correlation quotients (SURVEY.md
                section 9, U7) and pyramid values outside the guarded division range.

A fixture file holds the seeds and a SHA-256 of the image bytes, never the images: inputs() regenerates them and checks the digest.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile

import numpy as np

F32 = np.float32
LEVELS, FOVEA_LEVELS = 14, 7
CASES = {"A": dict(W=231, H=211, seed=9400, dark=None), "B": dict(W=333, H=251, seed=9401, dark=None),
         "C": dict(W=231, H=211, seed=9400, dark=9410)}
NONZERO_FILL = "7f7fffff"  # FLT_MAX in every new word of host memory: finite, so that a result that differs does so by arithmetic

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(_ROOT, "oracle", "_ref", "ref_driver")
GOLDEN = os.path.join(_ROOT, "tests", "golden")


def available():
    return os.access(DRIVER, os.X_OK)


def fixture_path(case, part):
    """tests/golden/ref_driver_<case>_<part>.npz; parts: "full" (the full-mode field), "fovea" (the stack and hierarchicalDisparity's field
    of it), and for case A "aux" (pyramid, taps, warped right image).  One file per part keeps every file under the size limit."""
    return os.path.join(GOLDEN, f"ref_driver_{case}_{part}.npz")


def parts(case):
    return ("full", "fovea", "aux") if case == "A" else ("full", "fovea")


def digest(L, R):
    return hashlib.sha256(np.ascontiguousarray(L).tobytes() + np.ascontiguousarray(R).tobytes()).hexdigest()


def inputs(case, sha256=None):
    """(left, right) rgb8 images of a case, contiguous; with `sha256`, checked against a fixture's record of them."""
    import dark_np
    from ug_stereomatcher_amd import synth
    c = CASES[case]
    L, R, _, _ = synth.make_pair(c["W"], c["H"], c["seed"])
    if c["dark"] is not None:
        L, R = dark_np.dark_pair(L, R, c["dark"])
    L, R = np.ascontiguousarray(L, np.uint8), np.ascontiguousarray(R, np.uint8)
    assert L.shape == R.shape == (c["H"], c["W"], 3)
    if sha256 is not None:
        assert digest(L, R) == str(sha256), f"case {case}: the regenerated images are not the ones the fixture was made from"
    return L, R


def header(case):
    """What every file of a case records about its inputs."""
    c = CASES[case]
    L, R = inputs(case)
    return dict(W=np.int32(c["W"]), H=np.int32(c["H"]), seed=np.int32(c["seed"]), dark_seed=np.int32(-1 if c["dark"] is None else c["dark"]),
                sha256=np.array(digest(L, R)))


def load(case):
    """The committed fixture of a case (all its parts) as a dict, and the images it was made from."""
    fx = {}
    want = header(case)
    for part in parts(case):
        with np.load(fixture_path(case, part)) as z:
            for k in want:
                assert str(z[k]) == str(want[k]), f"{fixture_path(case, part)}: {k} is {z[k]}, this tree makes {want[k]}"
            fx.update({k: z[k] for k in z.files})
    L, R = inputs(case, fx["sha256"])
    return fx, L, R


# ---- the child process ---------------------------------------------------------------------------------------------------------------------

def _read(path, n_planes=3):
    """A file of the driver cut by its own .dims record: a list of (n_planes, h, w) arrays, one per record."""
    with open(path + ".dims") as f:
        dims = [tuple(int(v) for v in line.split()) for line in f if line.strip()]
    raw = np.fromfile(path, F32)
    assert raw.size == sum(n_planes * w * h for w, h in dims), f"{path}: {raw.size} floats for {dims}"
    out, at = [], 0
    for w, h in dims:
        out.append(raw[at:at + n_planes * w * h].reshape(n_planes, h, w).copy())
        at += n_planes * w * h
    return out


def _run(args, host_fill=None, device_fill=None):
    env = dict(os.environ)
    for name, v in (("UGSM_REF_HOST_FILL", host_fill), ("UGSM_REF_DEVICE_FILL", device_fill)):
        env.pop(name, None)
        if v is not None:
            env[name] = v
    p = subprocess.run([DRIVER] + [str(a) for a in args], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
    if p.returncode != 0:
        raise RuntimeError(f"ref_driver {args[0]} ended with {p.returncode}: {p.stderr.decode(errors='replace')[-2000:]}")


class Session:
    """A scratch directory with the images of one pair in it; every method is one run of the driver."""

    def __init__(self, L, R):
        self.H, self.W, _ = L.shape
        self._tmp = tempfile.TemporaryDirectory(prefix="ref_driver_")
        self.dir = self._tmp.name
        np.ascontiguousarray(L, np.uint8).tofile(self._p("left.rgb"))
        np.ascontiguousarray(R, np.uint8).tofile(self._p("right.rgb"))

    def _p(self, name):
        return os.path.join(self.dir, name)

    def close(self):
        self._tmp.cleanup()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def match(self, fov=0, **fill):
        """match(L, R, fov) -> (3, H, W)"""
        out = self._p(f"match{fov}.f32")
        _run(["fovea" if fov else "full", self.W, self.H, self._p("left.rgb"), self._p("right.rgb"), out], **fill)
        (d,) = _read(out)
        return d

    def stack(self, **fill):
        """setFoveated(1), initStack, matchStackPyramid -> (3, F, fovH, fovW) in this project's layout; hierarchicalDisparity of it -> (3, H, W)"""
        out, out2 = self._p("stack.f32"), self._p("hier.f32")
        _run(["stack", self.W, self.H, self._p("left.rgb"), self._p("right.rgb"), out, out2], **fill)
        levels = _read(out)
        (d,) = _read(out2)
        return np.ascontiguousarray(np.stack(levels).transpose(1, 0, 2, 3)), d

    def pyramid(self):
        """CreatePyramidFromImage of the left image -> 14 arrays (3, h, w)"""
        out = self._p("pyr.f32")
        _run(["pyramid", self.W, self.H, self._p("left.rgb"), out])
        return _read(out)

    def taps(self):
        out = self._p("taps.f32")
        _run(["taps", out])
        return np.fromfile(out, F32)

    def warp_right(self, field):
        """warpRightImage(planes of the right image, field) -> (3, H, W)"""
        np.ascontiguousarray(field, F32).tofile(self._p("field.f32"))
        out = self._p("warp.f32")
        _run(["warp", self.W, self.H, self._p("right.rgb"), self._p("field.f32"), out])
        (w,) = _read(out)
        return w
