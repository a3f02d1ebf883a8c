#!/usr/bin/env python3
"""Writes tests/golden/ref_driver_*.npz: what the reference's own host driver gives for whole calls -- MatchGPULib.cpp with MatchLib.cu,
compiled for the CPU and run as oracle/_ref/ref_driver (oracle/Makefile ref-driver, oracle/ref_cpu/ref_driver.cpp) through
tests/ref_driver.py.  Needs the reference checkout: run where the build made oracle/_ref/.

Per case of tests/ref_driver.py (A 231 x 211, B 333 x 251, C the half-black pair at A's size), with the class's own MAX_LEVEL 14 and
foveatelevel 7:

  ref_driver_<case>_full.npz    full       match(L, R, 0): (3, H, W)
  ref_driver_<case>_fovea.npz   stack      setFoveated(1), initStack, matchStackPyramid: (3, 7, fovH, fovW), as the node packs it
                                fovea_full hierarchicalDisparity of that stack: (3, H, W); match(L, R, 1) is run as well and must
                                           give the same field, or nothing is written
  ref_driver_A_aux.npz          pyr0 (uint8: level 0 is the bytes themselves), pyr1 .. pyr13: CreatePyramidFromImage of the left image;
                                taps_bits: gaussiankernel's five taps as uint32; warp_right (uint8: the warp does no arithmetic on a
                                value): warpRightImage of the right planes by the full-mode field

Every file holds the seeds and a SHA-256 of the image bytes, not the images: tests regenerate them (ref_driver.inputs).

Time: one match() of the reference takes 55 to 65 s at 320 x 240 on an 8-core machine with nothing else running (the emulated blocks
of its shared-memory convolutions are real threads); the nine long runs of this script, four at a time, took 5 minutes.
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_driver as rd  # noqa: E402
from oracle import oracle as orc  # noqa: E402

PARALLEL = 4


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def save(case, part, **arrays):
    path = rd.fixture_path(case, part)
    np.savez_compressed(path, **rd.header(case), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {os.path.basename(path)}: {size} bytes")
    assert size < 1 << 20, "a committed file must stay under 1 MiB"


def main():
    orc.build()
    if not rd.available():
        raise SystemExit("oracle/_ref/ref_driver was not built: the reference checkout is not here")
    sessions = {case: rd.Session(*rd.inputs(case)) for case in rd.CASES}
    with ThreadPoolExecutor(PARALLEL) as pool:
        jobs = {}
        for case, s in sessions.items():
            jobs[case, "full"] = pool.submit(s.match, 0)
            jobs[case, "stack"] = pool.submit(s.stack)
            jobs[case, "fovea"] = pool.submit(s.match, 1)
        for case, s in sessions.items():
            full = jobs[case, "full"].result()
            stack, hier = jobs[case, "stack"].result()
            if not same(hier, jobs[case, "fovea"].result()):
                raise SystemExit(f"case {case}: match(L, R, 1) is not hierarchicalDisparity of matchStackPyramid's stack")
            save(case, "full", full=full)
            save(case, "fovea", stack=stack, fovea_full=hier)
            if case == "A":
                pyr = s.pyramid()
                warped = s.warp_right(full)
                assert len(pyr) == rd.LEVELS and (pyr[0] == pyr[0].astype(np.uint8)).all() and (warped == warped.astype(np.uint8)).all()
                save(case, "aux", pyr0=pyr[0].astype(np.uint8), **{f"pyr{k}": pyr[k] for k in range(1, rd.LEVELS)},
                     taps_bits=s.taps().view(np.uint32), warp_right=warped.astype(np.uint8))
    for s in sessions.values():
        s.close()


if __name__ == "__main__":
    main()
