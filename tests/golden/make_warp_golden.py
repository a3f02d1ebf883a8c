#!/usr/bin/env python3
"""Writes tests/golden/warp_right.npz: the right images of tests/warp_np.py's shapes warped by the reference's own `warp` stage (MatchLib.cu
compiled for the CPU, oracle/_ref/libmatchlib_cpu.so, through tests/ref_stages.py).  Needs the reference checkout: run where the build made
oracle/_ref/.  The file holds the seeds and the warped planes as uint8 (the sources are byte images and the warp does no arithmetic on a
value, so that is exact), not the inputs: tests regenerate those from the seeds (warp_np.fixture_inputs)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_stages as rs  # noqa: E402
import warp_np as wn  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    orc.build()
    ref = rs.load(orc)
    if ref is None:
        raise SystemExit("oracle/_ref/libmatchlib_cpu.so was not built: the reference checkout is not here")
    out = {"shapes": np.array(wn.SHAPES, np.int32), "pair_seed": np.int32(wn.PAIR_SEED), "field_seed": np.int32(wn.FIELD_SEED)}
    for k, (W, H) in enumerate(wn.SHAPES):
        _, R, d, wild = wn.fixture_inputs(k)
        for name, f in (("", d), ("_wild", wild)):
            if f is None:
                continue
            w = np.stack([ref.warp(p, f[0], f[1]) for p in wn.planes(R)])
            assert (w == w.astype(np.uint8)).all()
            out[f"{W}x{H}{name}"] = w.astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "warp_right.npz"), **out)
    print("wrote warp_right.npz:", os.path.getsize(os.path.join(HERE, "warp_right.npz")), "bytes")


if __name__ == "__main__":
    main()
