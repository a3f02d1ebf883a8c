"""The launch census: which kernels a call launches, level by level and in which groups, and what it writes.

The parity tests prove the bytes of every call mode; nothing in them proves that a change to the code that SEQUENCES a call (ugsm_levels.cpp:
run_level; ugsm_full.cpp: the descent; ugsm_fovea.cpp: the fovea phases) did not turn one batched launch into n launches or regroup them.
profile_events = 2 makes ugsm_get_kernel_stats report, per (kernel name, level) of slot 0, `launches` and `pixel_launches` -- the latter sums pixels x
entries of each launch, so it encodes the grouping.  One call at a time on a fresh one-slot context (so that `alone` is deterministic) gives one
census:

    {"launches": [[name, level, launches, pixel_launches], ...] sorted, launches > 0 only,
     "sha256":   [the SHA-256 of each output buffer's bytes, in the order the call was given them]}

An output buffer is a device buffer (the ugsm_submit_* calls) or a host array (the blocking and host-memory calls, HOST_CASES).  What a call
reads besides the images -- a prior field, a state, a prior stack -- is filled from numpy.random.default_rng(<a literal seed>): finite, never
zero (a zero prior would hide a dropped prior) and no other call's output (a case stands alone).

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
PRIOR_OFF = (40, -25)                                            # where a prior stack's window was matched: not at OFF_CENTRE

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


def _noise(seed, floats):
    """`floats` finite values, none of them zero: a prior, a state or a prior stack that is no call's output."""
    return np.random.default_rng(seed).uniform(0.25, 2.0, floats).astype(np.float32)


class _Run:
    """The buffers of one case: the images go up, the outputs -- device buffers, zeroed, or host arrays -- are hashed in the order given."""

    def __init__(self, c, lib):
        self.c, self.lib, self.held, self.outs = c, lib, [], []
        self.fw, self.fh = lib.fovea_dims(W, H, LEVELS, F)
        self.w, self.h = lib.level_dims(W, H, LEVELS)

    def images(self, n):
        dev = [(self.c.to_device(L), self.c.to_device(R)) for L, R in pairs()[:n]]
        self.held += [p for lr in dev for p in lr]
        return [l for l, _ in dev], [r for _, r in dev]

    def out(self, floats):
        p = self.given(np.zeros(floats, np.float32))
        self.outs.append(lambda: self.c.to_host(p, (floats,)))
        return p

    def given(self, arr):
        """A device buffer the call reads: not hashed."""
        p = self.c.to_device(arr)
        self.held.append(p)
        return p

    def host(self, arr):
        """A host array the call writes, hashed in its turn like a device buffer."""
        self.outs.append(lambda: arr)
        return arr

    def field(self):
        return self.out(3 * W * H)

    def stack(self):
        return self.out(3 * F * self.fh * self.fw)

    def level(self, e):
        return self.out(3 * self.w[e] * self.h[e])

    def finish(self):
        self.c.check(self.c.lib.ugsm_wait(self.c.handle, 0))
        sha = [hashlib.sha256(np.ascontiguousarray(get()).tobytes()).hexdigest() for get in self.outs]
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


def _full_checked(n, back):
    """back: the pairs whose right-to-left field the caller takes (the others' stay in the slot's LR buffer: its `kept` arithmetic)."""
    def run(r):
        dL, dR = r.images(n)
        outs = [r.field() for _ in range(n)]
        d_back = [r.field() if b in back else None for b in range(n)] if back else None
        r.c.submit_full_checked(0, dL, dR, W, H, 3 * W, outs, d_back, TAU)
    return run


def _seeded(n, start, seed):
    def run(r):
        dL, dR = r.images(n)
        priors = [r.given(_noise(seed + b, 3 * W * H)) for b in range(n)]
        r.c.submit_full_seeded(0, dL, dR, W, H, 3 * W, priors, start, [r.field() for _ in range(n)])
    return run


def _coarse(n, e, full):
    """full: the pairs that ask for the prolongation of their state."""
    def run(r):
        dL, dR = r.images(n)
        states = [r.level(e) for _ in range(n)]
        d_full = [r.field() if b in full else None for b in range(n)] if full else None
        r.c.submit_full_coarse(0, dL, dR, W, H, 3 * W, e, states, d_full)
    return run


def _fine(n, e, seed):
    def run(r):
        dL, dR = r.images(n)
        states = [r.given(_noise(seed + b, 3 * r.w[e] * r.h[e])) for b in range(n)]
        r.c.submit_full_fine(0, dL, dR, W, H, 3 * W, states, e, [r.field() for _ in range(n)])
    return run


def _fovea_warm1(r):
    """A prior stack matched at PRIOR_OFF, the new window at OFF_CENTRE, from fovea level 3."""
    dL, dR = r.images(1)
    prior = r.given(_noise(7411, 3 * F * r.fh * r.fw))
    r.c.submit_foveated_warm(0, dL, dR, W, H, 3 * W, [OFF_CENTRE], [prior], [PRIOR_OFF], 3, [r.stack()])


def _fovea_warm3_field(r):
    """Three pairs from full-resolution prior fields: more rows than travel in the launch's arguments (the slot's table)."""
    dL, dR = r.images(3)
    priors = [r.given(_noise(7421 + b, 3 * W * H)) for b in range(3)]
    r.c.submit_foveated_warm_field(0, dL, dR, W, H, 3 * W, OFFS3, priors, 0, [r.stack() for _ in range(3)])


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
    "full_checked_1": (_full_checked(1, ()), {}),
    "full_checked_3_some_back": (_full_checked(3, (0, 2)), {}),
    "seeded_1_s5": (_seeded(1, 5, 7401), {}),
    "seeded_3_s1": (_seeded(3, 1, 7402), {}),                                             # the pyramids stop at level max(start, 2) = 2
    "seeded_1_s13": (_seeded(1, LEVELS - 1, 7405), {}),                                   # the top level with a prior: no "top" iteration
    "coarse_1_e5_full": (_coarse(1, 5, (0,)), {}),
    "coarse_3_e2_some_full": (_coarse(3, 2, (0, 2)), {}),                                 # one prolong launch serves two entries
    "coarse_1_e0": (_coarse(1, 0, ()), {}),                                               # the whole call, on the direct-output path
    "fine_1_e5": (_fine(1, 5, 7406), {}),
    "fine_3_e1": (_fine(3, 1, 7407), {}),
    "fovea_warm_1_s3": (_fovea_warm1, {}),
    "fovea_warm_3_field_s0": (_fovea_warm3_field, {}),
}
DEV_CASES = ["full_1", "full_1_lr_full", "full_batch_3", "fovea_1_off_centre",            # (the checked calls refuse kernel_path 1)
             "seeded_3_s1", "coarse_3_e2_some_full", "fine_3_e1", "fovea_warm_3_field_s0"]


# ---- the blocking and host-memory calls: images and results in host memory, the results hashed as they lie there -------------------------
def _planes(a):
    return [a[c].ctypes.data for c in range(3)]


def _h_match_full(r):
    L, R = pairs()[0]
    out = r.host(np.zeros((3, H, W), np.float32))
    r.c.check(r.c.lib.ugsm_match_full(r.c.handle, L.ctypes.data, R.ctypes.data, W, H, 3 * W, *_planes(out)))


def _h_match_full_checked(r):
    fwd, bwd = r.c.match_full_checked(*pairs()[0], TAU, back=True)
    r.host(fwd), r.host(bwd)


def _h_match_full_seeded(r):
    r.host(r.c.match_full_seeded(*pairs()[0], _noise(7431, 3 * W * H).reshape(3, H, W), 4))


def _h_match_full_coarse(r):
    state, full = r.c.match_full_coarse(*pairs()[0], 3, want_full=True)
    r.host(state), r.host(full)


def _h_match_full_fine(r):
    r.host(r.c.match_full_fine(*pairs()[0], _noise(7432, 3 * r.w[3] * r.h[3]).reshape(3, r.h[3], r.w[3]), 3))


def _h_match_foveated(r):
    """With the left pyramid stack and without the right one: the offsets in the slot's result staging."""
    L, R = pairs()[0]
    stack = r.host(np.zeros((3, F, r.fh, r.fw), np.float32))
    pyrL = r.host(np.zeros((F, 3, r.fh, r.fw), np.float32))
    r.c.check(r.c.lib.ugsm_match_foveated(r.c.handle, L.ctypes.data, R.ctypes.data, W, H, 3 * W, OFF_CENTRE[0], OFF_CENTRE[1], *_planes(stack),
                                          pyrL.ctypes.data, None))


def _h_match_foveated_full(r):
    L, R = pairs()[0]
    out = r.host(np.zeros((3, H, W), np.float32))
    r.c.check(r.c.lib.ugsm_match_foveated_full(r.c.handle, L.ctypes.data, R.ctypes.data, W, H, 3 * W, OFF_CENTRE[0], OFF_CENTRE[1], *_planes(out)))


def _h_match_foveated_multi(tau):
    def run(r):
        for t in r.c.match_foveated_multi(*pairs()[1], OFFS3, tau):
            r.host(t)
    return run


def _h_match_foveated_warm(r):
    r.host(r.c.match_foveated_warm(*pairs()[0], _noise(7433, 3 * F * r.fh * r.fw).reshape(3, F, r.fh, r.fw), PRIOR_OFF, OFF_CENTRE, 2))


def _pinned_images(r, n):
    Ls, Rs = [], []
    for L, R in pairs()[:n]:
        for src, dst in ((L, Ls), (R, Rs)):
            a = r.c.host_array(src.shape, np.uint8)
            a[...] = src
            dst.append(a)
    return Ls, Rs


def _pinned_out(r, shape):
    a = r.c.host_array(shape)
    a[...] = 0
    return r.host(a)


def _h_full_batch_host(r):
    Ls, Rs = _pinned_images(r, 3)
    r.c.submit_full_batch_host(0, Ls, Rs, W, H, 3 * W, [_pinned_out(r, (3, H, W)) for _ in range(3)])


def _h_foveated_batch_host(r):
    Ls, Rs = _pinned_images(r, 3)
    r.c.submit_foveated_batch_host(0, Ls, Rs, W, H, 3 * W, OFFS3, [_pinned_out(r, (3, F, r.fh, r.fw)) for _ in range(3)])


# (under the default policy only)
HOST_CASES = {
    "match_full": (_h_match_full, {}),
    "match_full_checked": (_h_match_full_checked, {}),
    "match_full_seeded": (_h_match_full_seeded, {}),
    "match_full_coarse": (_h_match_full_coarse, {}),
    "match_full_fine": (_h_match_full_fine, {}),
    "match_foveated": (_h_match_foveated, {}),
    "match_foveated_full": (_h_match_foveated_full, {}),
    "match_foveated_multi": (_h_match_foveated_multi(None), {}),
    "match_foveated_multi_checked": (_h_match_foveated_multi(TAU), {}),
    "match_foveated_warm": (_h_match_foveated_warm, {}),
    "submit_full_batch_host": (_h_full_batch_host, {}),
    "submit_foveated_batch_host": (_h_foveated_batch_host, {}),
}


def case_ids():
    """(policy, case) of every census, in the order the golden file lists them."""
    return [(p, k) for p in POLICIES for k in CASES] + [("default", k) for k in HOST_CASES] + [(DEV_POLICY, k) for k in DEV_CASES]


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
    call, case_cfg = CASES[case] if case in CASES else HOST_CASES[case]
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
