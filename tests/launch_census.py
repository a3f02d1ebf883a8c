"""The launch census: which kernels a call launches, level by level and in which groups, and what it writes.

The parity tests prove the bytes of every call mode; nothing in them proves that a change to the code that SEQUENCES a call (ugsm_levels.cpp:
run_level; ugsm_full.cpp: the descent; ugsm_fovea.cpp: the fovea phases) did not turn one batched launch into n launches or regroup them.
profile_events = 2 makes ugsm_get_kernel_stats report, per (kernel name, level) of slot 0, `launches` and `pixel_launches` -- the latter sums pixels x
entries of each launch, so it encodes the grouping.  One call at a time on a fresh one-slot context (so that `alone` is deterministic) gives one
census:

    {"launches": [[name, level, launches, pixel_launches], ...] sorted, launches > 0 only,
     "sha256":   [the SHA-256 of each output buffer's bytes, in the order the call was given them]}

CLOUD_CASES does the same for row f-1 (ugsm_cloud.cpp): triangulation, the point clouds, the depth images and the queue's cloud calls, whose
launches the statistics time under the misc class with points = pairs x entries x sampled grid -- one batched cloud launch and n single ones
differ in `launches`.

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

    def out(self, floats, dtype=np.float32):
        p = self.given(np.zeros(floats, dtype))
        self.outs.append(lambda: self.c.to_host(p, (floats,), dtype))
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


# ---- row f-1: triangulation, the point clouds, the depth images (ugsm_cloud.cpp) and the queue's cloud calls ------------------------------------
# What such a call reads besides the left image is _noise: disparity planes or stacks and a confidence plane in 0.25 .. 2.0, so that min_conf =
# 1.0 keeps roughly half the points.  With the rig below the noise's Z has its 15th percentile at 210 and its 85th at 589: Z_WINDOW cuts both ends.  Every
# compact or windowed slot-level case keeps between 10 % and 90 % of its points by tests/cloud_np.py / depth_np.py (the queue's compact case by
# the CPU oracle's match of its pairs).  Every output is zeroed first and hashed whole: the points buffer (cap records), the count word, level or
# entry counts, the depth image and its valid counts.
MIN_CONF = 1.0
Z_WINDOW = (200.0, 600.0)
UNIT_16U = 0.05                                                  # 16UC1 holds Z * unit * 1000 below 65536: Z up to 1310 of this noise's 135 .. 866 (5 % .. 95 %)
Q_MIN_CONF = 0.7                                                 # a match's confidence, not noise: the queue's compact case
PCL32, XYZRGB16 = 0, 1                                           # UGSM_CLOUD_PCL32, UGSM_CLOUD_XYZRGB16
DEPTH_32F, DEPTH_16U = 0, 1                                      # UGSM_DEPTH_32F, UGSM_DEPTH_16U


def projections():
    """P1 and P2 of tests/test_gpu_cloud.py: the rectified 16 MP rig with its 0.12 baseline."""
    P1 = np.array([[7.3230899280915291e+03, 0., 2.4836974544986647e+03, 0.],
                   [0., 7.3035803715514758e+03, 1.7170248033347561e+03, 0.], [0., 0., 1., 0.]])
    P2 = P1.copy()
    P2[0, 3] = -7.3230899280915291e+03 * 0.12
    return P1, P2


def cloud_noise(seed, n):
    """dx, dy, conf of n values each from _noise; dx negated, so that the points lie in front of the rig (Z > 0: a depth image holds no other)."""
    a = _noise(seed, 3 * n)
    a[:n] *= -1
    return a


def _field_in(r, seed):
    """dx, dy, conf of W x H noise on the device and the left image of pair 0."""
    n = W * H
    p = r.given(cloud_noise(seed, n))
    return [p, p + 4 * n, p + 8 * n], r.images(1)[0][0]


def _stack_in(r, seed):
    """One stack of noise: the F levels of dx, of dy, of conf behind each other."""
    n = F * r.fw * r.fh
    p = r.given(cloud_noise(seed, n))
    return [p, p + 4 * n, p + 8 * n]


def _cloud_out(r, cap, fmt, counts=0):
    """The points buffer of cap records, the count word and `counts` level or entry counts (0: none)."""
    pts, cnt = r.out(cap * (32 if fmt == PCL32 else 16), np.uint8), r.out(1, np.int64)
    return (pts, cap, cnt) + ((r.out(counts, np.int64),) if counts else ())


def _params(r, fmt, s=1, compact=False, window=False):
    kw = dict(min_conf=MIN_CONF) if compact else {}
    if window:
        kw.update(z_min=Z_WINDOW[0], z_max=Z_WINDOW[1])
    return r.lib.cloud_params(sampling=s, format=fmt, compact=compact, **kw)


def _triangulate(r):
    (dx, dy, _), _ = _field_in(r, 7501)
    r.c.triangulate(dx, dy, W, H, *projections(), r.out(3 * W * H))


def _triangulate_fovea(r):
    sx, sy, _ = _stack_in(r, 7502)
    r.c.triangulate_fovea(sx, sy, r.fw, r.fh, 2, *r.lib.fovea_level_mapping(W, H, LEVELS, F, 2, OFF_CENTRE), *projections(), r.out(3 * r.fw * r.fh))


def _cloud(fmt, s=1, compact=False, window=False, cap_div=1, seed=7503):
    def run(r):
        planes, rgb = _field_in(r, seed)
        cap = r.lib.cloud_points(W, H, s) // cap_div
        r.c.point_cloud(*planes, rgb, W, H, 3 * W, *projections(), _params(r, fmt, s, compact, window), *_cloud_out(r, cap, fmt))
    return run


def _cloud_fovea(level, compact, seed=7504):
    def run(r):
        stack, rgb = _stack_in(r, seed), r.images(1)[0][0]
        r.c.point_cloud_fovea(*stack, r.fw, r.fh, level, *r.lib.fovea_level_mapping(W, H, LEVELS, F, level, OFF_CENTRE), rgb, W, H, 3 * W,
                              *projections(), _params(r, PCL32, 1, compact), *_cloud_out(r, r.fw * r.fh, PCL32))
    return run


def _cloud_resized(r):
    planes, rgb = _field_in(r, 7505)
    r.c.point_cloud_resized(*planes, rgb, W, H, 3 * W, *projections(), 0.2, _params(r, PCL32), *_cloud_out(r, r.lib.resized_cloud_points(W, H, 0.2), PCL32))


def _cloud_resized_fovea(r):
    stack, rgb = _stack_in(r, 7506), r.images(1)[0][0]
    r.c.point_cloud_resized_fovea(*stack, r.fw, r.fh, 2, *r.lib.fovea_level_mapping(W, H, LEVELS, F, 2, OFF_CENTRE), rgb, W, H, 3 * W, *projections(),
                                  0.5, _params(r, XYZRGB16, 1, True), *_cloud_out(r, r.lib.resized_cloud_points(r.fw, r.fh, 0.5), XYZRGB16),
                                  colour_mapped=True)


def _cloud_fovea_all(compact, seed=7507):
    def run(r):
        stack, rgb = _stack_in(r, seed), r.images(1)[0][0]
        cap = r.lib.fovea_cloud_points(W, H, LEVELS, F, OFF_CENTRE, 1)
        r.c.point_cloud_fovea_all(*stack, W, H, OFF_CENTRE, rgb, 3 * W, *projections(), _params(r, PCL32, 1, compact), *_cloud_out(r, cap, PCL32, F))
    return run


def _cloud_fovea_multi(compact, seed=7508):
    def run(r):
        stacks, rgb = [_stack_in(r, seed + j)[0] for j in range(len(OFFS3))], r.images(1)[0][0]
        cap = r.lib.fovea_multi_cloud_points(W, H, LEVELS, F, OFFS3, 1)
        r.c.point_cloud_fovea_multi(stacks, W, H, OFFS3, rgb, 3 * W, *projections(), _params(r, XYZRGB16, 1, compact),
                                    *_cloud_out(r, cap, XYZRGB16, (F - 1) * len(OFFS3) + 1))
    return run


def _depth(fmt, factor=1.0, conf=False, seed=7511):
    def run(r):
        (dx, dy, c), _ = _field_in(r, seed)
        p = r.lib.depth_params(format=fmt, unit=UNIT_16U if fmt == DEPTH_16U else None, factor=factor, min_conf=MIN_CONF if conf else None)
        dw, dh = r.lib.depth_image_size(W, H, factor)
        r.c.depth_image(dx, dy, c if conf else None, W, H, *projections(), p, r.out(dw * dh, np.uint16 if fmt == DEPTH_16U else np.float32),
                        r.out(1, np.uint64))
    return run


def _depth_fovea(fmt, level, seed=7512):
    def run(r):
        sx, sy, _ = _stack_in(r, seed)
        n = F if level == r.lib.UGSM_DEPTH_ALL_LEVELS else 1
        r.c.depth_image_fovea(sx, sy, None, W, H, OFF_CENTRE, level, *projections(), r.lib.depth_params(format=fmt, unit=UNIT_16U if fmt == DEPTH_16U else None),
                              r.out(n * r.fw * r.fh, np.uint16 if fmt == DEPTH_16U else np.float32), r.out(n, np.uint64))
    return run


def _depth_fovea_all(r):
    _depth_fovea(DEPTH_16U, r.lib.UGSM_DEPTH_ALL_LEVELS, 7513)(r)


def _h_match_full_depth(r):
    depth, planes = r.c.match_full_depth(*pairs()[0], *projections(), r.lib.depth_params(), planes=True)
    r.host(depth), r.host(planes)


# ... the queue's cloud calls: n pairs enqueued on the one-slot context with batch = 4, flushed, drained with next_done; a managed pair's lent
# buffers are copied (and hashed in their turn) before the next next_done
def _spec(r, fmt=PCL32, compact=False, want_planes=False):
    p = r.lib.cloud_params(format=fmt, compact=compact, min_conf=Q_MIN_CONF if compact else None)
    return r.lib.queue_cloud(*projections(), p, want_planes=want_planes)


def _drain(r, n, each=None):
    r.c.flush()
    for tag in range(n):
        d = r.c.next_done(True)
        assert d is not None and d.tag == tag, (tag, d and d.tag)
        if each:
            each(d)
    assert r.c.next_done(True) is None


def _q_cloud_dev(n, fovea=False, compact=False, lr=False, checked=False):
    def run(r):
        if lr:
            r.c.set_lr_check(TAU, r.lib.UGSM_LR_FULL)
        dL, dR = r.images(n)
        spec = _spec(r, PCL32, compact)
        for b in range(n):
            if fovea:
                cap = r.lib.fovea_cloud_points(W, H, LEVELS, F, OFFS3[b], 1)
                pts, cap, cnt, lvl = _cloud_out(r, cap, PCL32, F)
                r.c.enqueue_foveated_cloud(dL[b], dR[b], W, H, 3 * W, OFFS3[b], r.stack(), spec, pts, cap, cnt, b, d_level_counts=lvl)
            elif checked:
                out, back = r.field(), (r.field() if b == 0 else None)      # (pair 1's right-to-left field stays in the slot)
                r.c.enqueue_full_checked_cloud(dL[b], dR[b], W, H, 3 * W, out, back, TAU, spec, *_cloud_out(r, W * H, PCL32), b)
            else:
                r.c.enqueue_full_cloud(dL[b], dR[b], W, H, 3 * W, r.field(), spec, *_cloud_out(r, W * H, PCL32), b)
        _drain(r, n)
    return run


def _lent_cloud(r):
    rec, count, levels = r.c.done_cloud()
    r.host(rec.view(np.uint8).copy()), r.host(np.array([count] + levels, np.int64))


def _q_cloud_managed(n, fovea=False, want_planes=False):
    def run(r):
        spec = _spec(r, PCL32, False, want_planes)
        for b in range(n):
            L, R = pairs()[b]
            if fovea:
                r.c.enqueue_foveated_cloud_managed(L, R, OFF_CENTRE, spec, b)
            else:
                r.c.enqueue_full_cloud_managed(L, R, spec, b)

        def each(d):
            if want_planes:
                for p in r.c.managed_planes(d, [(H, W)] * 3):
                    r.host(p.copy())
            _lent_cloud(r)
        _drain(r, n, each)
    return run


def _q_checked_cloud_managed_back(r):
    spec = _spec(r)
    for b in range(2):
        r.c.enqueue_full_checked_cloud_managed(*pairs()[b], TAU, True, spec, b)

    def each(d):
        fwd, bwd, back = r.c.done_checked((H, W))
        r.host(np.array([fwd, bwd], np.int64)), r.host(back)
        _lent_cloud(r)
    _drain(r, 2, each)


# (under the default policy only)
CLOUD_CASES = {
    "triangulate": (_triangulate, {}),
    "triangulate_fovea": (_triangulate_fovea, {}),
    "cloud_dense_pcl32": (_cloud(PCL32), {}),
    "cloud_compact_xyzrgb16_s3": (_cloud(XYZRGB16, 3, True, True), {}),
    "cloud_dense_cap_half": (_cloud(PCL32, cap_div=2), {}),                              # the o >= cap path; the count beyond cap
    "cloud_fovea_l2_dense": (_cloud_fovea(2, False), {}),
    "cloud_fovea_l2_compact": (_cloud_fovea(2, True), {}),
    "cloud_resized_f02_dense": (_cloud_resized, {}),
    "cloud_resized_fovea_f05_compact_mapped": (_cloud_resized_fovea, {}),
    "cloud_fovea_all_dense": (_cloud_fovea_all(False), {}),
    "cloud_fovea_all_compact": (_cloud_fovea_all(True), {}),
    "cloud_fovea_multi_dense": (_cloud_fovea_multi(False), {}),
    "cloud_fovea_multi_compact": (_cloud_fovea_multi(True), {}),
    "depth_32f": (_depth(DEPTH_32F), {}),
    "depth_16u_resized_f05": (_depth(DEPTH_16U, 0.5, True), {}),
    "depth_fovea_l3_32f": (_depth_fovea(DEPTH_32F, 3), {}),
    "depth_fovea_all_16u": (_depth_fovea_all, {}),
    "match_full_depth": (_h_match_full_depth, {}),
    "q_full_cloud_dev_3": (_q_cloud_dev(3), dict(batch=4)),                              # lockstep: one cloud launch for three pairs
    "q_fovea_cloud_dev_3_compact": (_q_cloud_dev(3, fovea=True, compact=True), dict(batch=4)),
    "q_full_cloud_managed_3_planes": (_q_cloud_managed(3, want_planes=True), dict(batch=4)),
    "q_fovea_cloud_managed_1": (_q_cloud_managed(1, fovea=True), dict(batch=4)),         # pair by pair
    "q_full_cloud_dev_2_lr": (_q_cloud_dev(2, lr=True), dict(batch=4)),                  # the matcher, so the clouds, pair by pair
    "q_full_checked_cloud_dev_2": (_q_cloud_dev(2, checked=True), dict(batch=4)),
    "q_full_checked_cloud_managed_2_back": (_q_checked_cloud_managed_back, dict(batch=4)),
}


def case_ids():
    """(policy, case) of every census, in the order the golden file lists them."""
    return ([(p, k) for p in POLICIES for k in CASES] + [("default", k) for k in HOST_CASES] + [(DEV_POLICY, k) for k in DEV_CASES]
            + [("default", k) for k in CLOUD_CASES])


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
    call, case_cfg = next(t[case] for t in (CASES, HOST_CASES, CLOUD_CASES) if case in t)
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
