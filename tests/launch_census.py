"""The launch census: which kernels a call launches, level by level and in which groups, and what it writes.

The parity tests prove the bytes of every call mode; nothing in them proves that a change to the code that SEQUENCES a call (ugsm_runtime.cpp:
run_level, the descent, the fovea phases) did not turn one batched launch into n launches or regroup them.  profile_events = 2 makes
ugsm_get_kernel_stats report, per (kernel name, level) of slot 0, `launches` and `pixel_launches` -- the latter sums pixels x entries of each
launch, so it encodes the grouping.  One call at a time on a fresh one-slot context (so that `alone` is deterministic) gives one census:

    {"launches": [[name, level, launches, pixel_launches], ...] sorted, launches > 0 only,
     "sha256":   [the SHA-256 of each output buffer's bytes, in the order the call was given them]}

tests/golden/make_launch_census.py records the census of every case into tests/golden/launch_census.json on a build of the commit the
refactoring started from; tests/test_gpu_launch_census.py asserts the code under test gives the same, case by case.  Both take their cases
from here, so they cannot drift.
"""
import contextlib
import hashlib
import os

import numpy as np

W, H, LEVELS, F = 333, 251, 14, 7     # the size of tests/golden/ref_driver_B_*: every one of the 14 levels exists at it
TAU = 1.0
OFF_CENTRE = (-60, 35)
OFFS3 = [(0, 0), OFF_CENTRE, (5000, -5000)]                      # centred, off-centre, clamped into a corner
OFFS16 = [(17 * j - 120, 90 - 11 * j) for j in range(16)]

# policy -> (ugsm_config fields, development overrides read at ugsm_create under UGSM_DEV=1)
POLICIES = {
    "default": ({}, {}),
    "march": (dict(march_min_pixels=1), {}),                                            # every level through k_cost_march, seeded form included
    "march4": (dict(small_max_pixels=-1), {"UGSM_MARCH4": "1,2000000000"}),             # ... through k_cost_march4
}
DEV_POLICY = "dev_kernel_path1"                                                          # libugsm_dev.so, one kernel per reference stage

_PAIRS = []


def pairs():
    """Three pairs; the second has a zero patch in its left image (0 / 0 -> NaN correlations), as tests/test_gpu_fovea_multi.py::_pair."""
    if not _PAIRS:
        from ug_stereomatcher_amd import synth
        for j in range(3):
            L, R = synth.make_pair(W, H, synth.BASE_SEED + 7300 + 11 * j)[:2]
            if j == 1:
                L = L.copy()
                L[H // 5:H // 5 + 24, W // 4:W // 4 + 40] = 0
            _PAIRS.append((np.ascontiguousarray(L), np.ascontiguousarray(R)))
    return _PAIRS


class _Run:
    """Device buffers of one case: the images go up, the outputs are zeroed, read back in order and hashed."""

    def __init__(self, c, lib):
        self.c, self.lib, self.held, self.outs = c, lib, [], []
        self.fw, self.fh = lib.fovea_dims(W, H, LEVELS, F)

    def images(self, n):
        dev = [(self.c.to_device(L), self.c.to_device(R)) for L, R in pairs()[:n]]
        self.held += [p for lr in dev for p in lr]
        return [l for l, _ in dev], [r for _, r in dev]

    def out(self, floats):
        p = self.c.to_device(np.zeros(floats, np.float32))
        self.held.append(p)
        self.outs.append((p, floats))
        return p

    def field(self):
        return self.out(3 * W * H)

    def stack(self):
        return self.out(3 * F * self.fh * self.fw)

    def finish(self):
        self.c.check(self.c.lib.ugsm_wait(self.c.handle, 0))
        sha = [hashlib.sha256(self.c.to_host(p, (n,)).tobytes()).hexdigest() for p, n in self.outs]
        for p in self.held:
            self.c.free(p)
        return sha


def _full1(r):
    dL, dR = r.images(1)
    r.c.check(r.c.lib.ugsm_submit_full(r.c.handle, 0, dL[0], dR[0], W, H, 3 * W, r.field()))


def _full1_lr(r):
    r.c.set_lr_check(TAU, r.lib.UGSM_LR_FULL)
    _full1(r)


def _full3(r):
    dL, dR = r.images(3)
    r.c.submit_full_batch(0, dL, dR, W, H, 3 * W, [r.field() for _ in range(3)])


def _fovea1(r):
    dL, dR = r.images(1)
    r.c.check(r.c.lib.ugsm_submit_foveated(r.c.handle, 0, dL[0], dR[0], W, H, 3 * W, OFF_CENTRE[0], OFF_CENTRE[1], r.stack(), None, None))


def _fovea3_some_pyramids(r):
    """Both pyramid stacks for pairs 0 and 2 only: the fine phase's `all == false` branch."""
    dL, dR = r.images(3)
    stacks = [r.stack() for _ in range(3)]
    pL = [r.stack(), None, r.stack()]
    pR = [r.stack(), None, r.stack()]
    r.c.submit_foveated_batch(0, dL, dR, W, H, 3 * W, OFFS3, stacks, pL, pR)


def _fovea2_lr(r):
    r.c.set_lr_check(TAU, r.lib.UGSM_LR_FOVEATED)
    dL, dR = r.images(2)
    r.c.submit_foveated_batch(0, dL, dR, W, H, 3 * W, OFFS3[:2], [r.stack() for _ in range(2)])


def _multi(offs, tau=None, pair=1):
    def run(r):
        dL, dR = r.images(pair + 1)
        stacks = [r.stack() for _ in offs]
        if tau is None:
            r.c.submit_foveated_multi(0, dL[pair], dR[pair], W, H, 3 * W, offs, stacks)
        else:
            r.c.submit_foveated_multi_checked(0, dL[pair], dR[pair], W, H, 3 * W, offs, stacks, tau)
    return run


# name -> (the call, further ugsm_config fields)
CASES = {
    "full_1": (_full1, {}),
    "full_1_lr_full": (_full1_lr, {}),
    "full_batch_3": (_full3, {}),
    "fovea_1_off_centre": (_fovea1, {}),
    "fovea_batch_3_some_pyramid_stacks": (_fovea3_some_pyramids, {}),
    "fovea_batch_2_lr_fovea": (_fovea2_lr, {}),
    "multi_1": (_multi(OFFS3[1:2]), {}),
    "multi_3": (_multi(OFFS3), {}),
    "multi_3_early_exit": (_multi(OFFS3), dict(early_exit_threshold=0.02)),               # window by window
    "multi_checked_3": (_multi(OFFS3, TAU), {}),
    "multi_checked_16": (_multi(OFFS16, TAU), {}),                                        # 32 entries: two launches of 16; K-cost per direction
}
DEV_CASES = list(CASES)[:4]


def case_ids():
    """(policy, case) of every census, in the order the golden file lists them."""
    return [(p, k) for p in POLICIES for k in CASES] + [(DEV_POLICY, k) for k in DEV_CASES]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in list(env) + ["UGSM_DEV"]}
    os.environ.update(env, UGSM_DEV="1")
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def census(lib, policy, case):
    """The census of one case under one policy, taken on a fresh one-slot context."""
    call, case_cfg = CASES[case]
    cfg, env = (dict(kernel_path=1, dev=True), {}) if policy == DEV_POLICY else POLICIES[policy]
    with _environ(env):
        c = lib.Context(levels=LEVELS, fovea_levels=F, slots=1, profile_events=2, **dict(cfg, **case_cfg))
    with c:
        r = _Run(c, lib)
        call(r)
        sha = r.finish()
        rows = sorted([s["name"], s["level"], s["launches"], _number(s["pixel_launches"])] for s in c.kernel_stats() if s["launches"] > 0)
    return {"launches": rows, "sha256": sha}


def _number(x):
    return int(x) if float(x).is_integer() else float(x)
