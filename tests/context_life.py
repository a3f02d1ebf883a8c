"""One context through calls of changing size, kind and format (test infrastructure; no tests in here).

A node creates one context and keeps it for life; the calls meet in the slot (csrc/ugsm_slot.hpp), which carries sizes, strides, capacities, the
layout of its result staging and a dozen flags from one call to the next.  This file is the vocabulary for scripts of such calls and the runner that
plays a script on ONE context:

    step(kind, frame, pairs, slot, wait, src, **args)    one call: its kind, frame ("A", "B", ..), image pairs (seeds), slot, whether the slot is
                                                         waited for behind it, the earlier step whose DEVICE output it reads, its parameters
    Expect(orc)                                          what every step must write, from the CPU oracle and the restatements the per-feature tests
                                                         use, computed once per distinct case (key()) and shared
    play(lib, c, exp, script)                            stages every buffer of the script first, then submits the calls back to back -- a step
                                                         without wait_after is followed at once by the next call on its slot --, waits once per
                                                         slot, compares every output bit for bit, checks guard bands and inputs
    transitions(script) / walk(seed)                     what a script exercises per slot, computed from its steps; the random walks

Every output lies in a buffer of its own, filled with the poison byte of tests/guarded.py; device float buffers lie between its guard bands.
Settings (input format, LR check) are followed through the script: a step is staged in the format in force when it is submitted and expected
under the settings it captures.  On a mismatch the failing step is played alone on a fresh context, and the message says which of the two it is:
wrong there too (the step itself) or right there (what an earlier call left in the slot)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import cloud_np as cn
import coarse_np as cs
import depth_np as dn
import encode_np as en
import float_np as fl
import fovea_seeded_np as fs
import reconstruct_multi_np as rm
import seeded_np as sn
import warp_np as wn
from conftest import assert_bit_equal
from guarded import POISON, Guards
from test_gpu_cloud import P1, P2A
from test_gpu_lr_fovea import _checked as checked_stack
from test_gpu_warp import _wd as residual_quotient

LEVELS, FOVEA = 9, 4
MAIN = dict(levels=LEVELS, fovea_levels=FOVEA, slots=2, batch=4)
SHARED = dict(levels=LEVELS, fovea_levels=FOVEA, slots=3, streams=1, batch=4)   # one stream for three slots: ugsm_wait goes by ev_done
FRAMES = {"A": (203, 149), "B": (333, 251), "C": (640, 480), "T": (97, 401), "Wd": (801, 90)}
SEED = 7000                     # + the pair's number: synth.make_pair(W, H, synth.BASE_SEED + SEED + pair)
TAU = 1.0                       # the LR threshold (tests/test_gpu_lr_full.py's); test_context_life_host.py asserts it fires and spares
EXTRA = 64                      # records / elements of poison behind a cloud or a depth image
RGB8, BGR8, MONO8, RGB32F = en.RGB8, en.BGR8, en.MONO8, fl.RGB32F
FORMAT_NAMES = {**en.NAMES, **fl.NAMES}
OK, BAD_ARG, SIZE_MISMATCH, TOO_SMALL, STATE, NOMEM = 0, 1, 2, 3, 7, 6
ITER = (4, 5, 0, 1, 2)          # stage_iterate: mi, S, is_top, m_from, m_to (tests/test_gpu_parity.py's short run)
SMOOTH = (5, 1)                 # stage_smooth: passes, box

# kind -> (family, pairs it brings, blocking: runs on slot 0 and returns finished)
KINDS = {
    "full": ("full", 1, False), "full_batch": ("full", None, False), "full_host": ("full", 1, True), "full_batch_host": ("full", None, False),
    "full_checked": ("full", None, False), "full_seeded": ("full", 1, False), "coarse": ("full", 1, False), "fine": ("full", 0, False),
    "fov_batch": ("fovea", None, False), "fov_host": ("fovea", 1, True), "fov_multi": ("fovea", 1, False), "fov_multi_checked": ("fovea", 1, False),
    "fov_warm": ("fovea", 1, False), "pyramids": ("phase", 1, False), "fovea_coarse": ("phase", 0, False), "fovea_fine": ("phase", 0, False),
    "cloud": ("post", 0, False), "depth16u": ("post", 0, False), "warp_right": ("post", 0, False), "residual": ("post", 0, False),
    "stage_iterate": ("stage", 1, True), "stage_smooth": ("stage", 1, True), "stage_pyramid": ("stage", 1, True),
    "set_format": ("setting", 0, False), "set_lr": ("setting", 0, False), "refused": ("refused", 1, False),
}
LR_FULL_KINDS = {"full", "full_host", "full_batch", "full_batch_host", "full_seeded", "coarse", "fine"}   # what ugsm_set_lr_check(tau, UGSM_LR_FULL) changes
HOST_KINDS = {"full_host", "fov_host"}                                     # the blocking calls on caller host memory: hout / hpin laid out their way
BUILDS_PYRAMIDS = {k for k, v in KINDS.items() if v[0] in ("full", "fovea") or k in ("pyramids", "stage_pyramid")}


@dataclass(frozen=True)
class Step:
    kind: str
    frame: str = "B"
    pairs: tuple = ()       # the image pairs the step brings, by number
    args: tuple = ()        # the kind's parameters: sorted (name, value) items
    slot: int = 0
    wait_after: bool = True
    src: int = -1           # the earlier step (index in the script) whose device output, or pyramids, this one works on

    def arg(self, name, default=None):
        return dict(self.args).get(name, default)

    @property
    def size(self):
        return FRAMES[self.frame]

    @property
    def n(self):
        return max(len(self.pairs), 1)

    def __str__(self):
        a = ", ".join(f"{k}={v}" for k, v in self.args)
        return f"{self.kind}({a}) {self.frame} {self.size[0]}x{self.size[1]} pairs {list(self.pairs)} slot {self.slot}{'' if self.wait_after else ' no wait'}"


def step(kind, frame="B", pairs=(), slot=0, wait=True, src=-1, **args):
    fam, brings, blocking = KINDS[kind]
    pairs = (pairs,) if isinstance(pairs, int) else tuple(pairs)
    assert brings is None or len(pairs) == brings, (kind, pairs)
    assert not blocking or slot == 0, f"{kind} runs on slot 0"
    return Step(kind, frame, pairs, tuple(sorted(args.items())), slot, bool(wait) or blocking, src)


# ---- what a script says about itself ----------------------------------------------------------------------------------------------------

def settings(script):
    """(input format, LR tau, LR modes) in force when each step is submitted; a context starts at rgb8, check off."""
    fmt, tau, modes, out = RGB8, 0.0, 1, []
    for s in script:
        out.append((fmt, tau, modes))
        if s.kind == "set_format":
            fmt = s.arg("fmt")
        elif s.kind == "set_lr":
            tau, modes = s.arg("tau"), s.arg("modes")
    return out


def lr_on(setting):
    return setting[1] > 0 and bool(setting[2] & 1)


def pair_of(script, i):
    """The pairs a step works on: its own, or those of the step it hangs on."""
    while not script[i].pairs and script[i].src >= 0:
        i = script[i].src
    return script[i].pairs


def transitions(script):
    """Per slot, what the script makes the slot go through -- {slot: {name: count}} -- computed from the steps alone:
      grow_behind_unwaited   a call of a larger frame right behind an unwaited call of a smaller one
      shrink_warm            a smaller frame on a slot that has held a larger one
      nb_down / nb_up        fewer / more pairs than the call before
      checked_to_plain       a plain full-mode call behind a checked one
      fovea_to_full / full_to_fovea, host_to_slot / slot_to_host (the blocking host-memory calls against the slot-level ones)
      format_behind_unwaited a change of input format right behind an unwaited submit (on any slot: the setting is the context's)
      lr_behind_unwaited     the same for the LR check
      post_shrink / post_grow a cloud, depth image, warp or residual of a smaller frame than one before it / a larger one than the last
      no_wait                hand-overs: a call submitted behind an unwaited one"""
    out, last, biggest, post = {}, {}, {}, {}
    prev_any = None
    for s in script:
        fam = KINDS[s.kind][0]
        if fam == "setting":
            if prev_any is not None and not prev_any.wait_after:
                t = out.setdefault(prev_any.slot, {})
                name = "format_behind_unwaited" if s.kind == "set_format" else "lr_behind_unwaited"
                t[name] = t.get(name, 0) + 1
            continue
        t = out.setdefault(s.slot, {})

        def hit(name):
            t[name] = t.get(name, 0) + 1
        p = last.get(s.slot)
        px = s.size[0] * s.size[1]
        if p is not None:
            ppx = p.size[0] * p.size[1]
            if not p.wait_after:
                hit("no_wait")
                if px > ppx and s.kind in BUILDS_PYRAMIDS and p.kind in BUILDS_PYRAMIDS:
                    hit("grow_behind_unwaited")
            if s.kind in BUILDS_PYRAMIDS and p.kind in BUILDS_PYRAMIDS:
                if s.n < p.n:
                    hit("nb_down")
                if s.n > p.n:
                    hit("nb_up")
            pf = KINDS[p.kind][0]
            if p.kind == "full_checked" and fam == "full" and s.kind != "full_checked":
                hit("checked_to_plain")
            if pf in ("fovea", "phase") and fam == "full":
                hit("fovea_to_full")
            if pf == "full" and fam in ("fovea", "phase"):
                hit("full_to_fovea")
            if p.kind in HOST_KINDS and s.kind not in HOST_KINDS and fam in ("full", "fovea"):
                hit("host_to_slot")
            if s.kind in HOST_KINDS and p.kind not in HOST_KINDS and pf in ("full", "fovea"):
                hit("slot_to_host")
        if s.kind in BUILDS_PYRAMIDS and px < biggest.get(s.slot, 0):
            hit("shrink_warm")
        if fam == "post":                                                  # (the count buffer, the residual's rows: grown on demand, per kind)
            seen_px = post.setdefault((s.slot, s.kind), [])
            if seen_px and px < max(seen_px):
                hit("post_shrink")
            if seen_px and px > seen_px[-1]:
                hit("post_grow")
            seen_px.append(px)
        if s.kind in BUILDS_PYRAMIDS:
            biggest[s.slot] = max(biggest.get(s.slot, 0), px)
        last[s.slot] = s
        prev_any = s
    return out


# ---- the expected values ----------------------------------------------------------------------------------------------------------------

def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, (tuple, list)):
        for x in v:
            _freeze(x)
    elif isinstance(v, dict):
        for x in v.values():
            _freeze(x)
    return v


def _cls(fmt):
    return "mono" if fmt in (MONO8, fl.MONO32F) else "rgb"


def encode(img, fmt):
    """The rgb8 image `img` as the caller hands it over in `fmt`."""
    return fl.encode(img, fmt) if fmt in fl.FORMATS else en.encode(img, fmt)


def percentile_window(z, lo=10, hi=90):
    zf = z[np.isfinite(z)]
    return float(np.percentile(zf, lo)), float(np.percentile(zf, hi))


class Expect:
    """Expected values by the CPU oracle and the per-feature restatements, once per distinct case: key(script, i) names the case -- kind, frame,
    pairs, parameters, what the settings make of it, and the case it hangs on."""

    def __init__(self, orc):
        self.orc, self.memo, self.computed = orc, {}, 0

    def _m(self, key, f):
        if key not in self.memo:
            self.memo[key] = _freeze(f())
            self.computed += 1
        return self.memo[key]

    # the images and what the oracle makes of them
    def images(self, frame, p):
        def make():
            from ug_stereomatcher_amd import synth
            return synth.make_pair(*FRAMES[frame], synth.BASE_SEED + SEED + p)[:2]
        return self._m(("img", frame, p), make)

    def seen(self, frame, p, fmt):
        """The rgb8 pair a call in `fmt` is defined on: the conversion of what the caller hands over (mono: channel 0 three times)."""
        L, R = self.images(frame, p)
        if _cls(fmt) == "rgb":
            return L, R
        return self._m(("mono", frame, p), lambda: tuple(en.to_rgb8(en.encode(a, MONO8), MONO8) for a in (L, R)))

    def pyr(self, frame, p, fmt):
        return self._m(("pyr", frame, p, _cls(fmt)), lambda: sn.pyramids(self.orc, *self.seen(frame, p, fmt), LEVELS))

    def full(self, frame, p, fmt, back=False):
        L, R = self.seen(frame, p, fmt)
        return self._m(("full", frame, p, _cls(fmt), back), lambda: self.orc.match_full(R, L, LEVELS) if back else self.orc.match_full(L, R, LEVELS))

    def checked(self, frame, p, fmt, tau):
        """(out, back, (marked forward, marked backward)): dx, dy of the unchecked fields, the confidences checked against the other direction."""
        def make():
            F, B = self.full(frame, p, fmt), self.full(frame, p, fmt, True)
            cF, nF = self.orc.lr_check(F, B, tau)
            cB, nB = self.orc.lr_check(B, F, tau)
            return (np.stack([F[0], F[1], cF[2]]), np.stack([B[0], B[1], cB[2]]), (int(nF), int(nB)))
        return self._m(("checked", frame, p, _cls(fmt), tau), make)

    def fov(self, frame, p, fmt, off, back=False):
        L, R = self.seen(frame, p, fmt)
        if back:
            return self._m(("fovb", frame, p, _cls(fmt), off), lambda: self.orc.match_foveated(R, L, LEVELS, FOVEA, off[0], off[1])[0])
        return self._m(("fov", frame, p, _cls(fmt), off), lambda: self.orc.match_foveated(L, R, LEVELS, FOVEA, off[0], off[1], want_pyr=True))

    def fov_checked(self, frame, p, fmt, off, tau):
        def make():
            chk, counts = checked_stack(self.orc, self.fov(frame, p, fmt, off)[0], self.fov(frame, p, fmt, off, True), tau)
            return chk, [int(m) for m in counts]
        return self._m(("fovc", frame, p, _cls(fmt), off, tau), make)

    def cloud_params(self, planes):
        """min_conf and the Z window of a compact cloud, from the restatement's own percentiles."""
        z = self.orc.triangulate(planes[0], planes[1], P1, P2A)[2]
        lo, hi = percentile_window(z)
        return dict(min_conf=float(np.percentile(planes[2][np.isfinite(planes[2])], 30)), z_min=lo, z_max=hi)

    def depth_params(self, planes):
        z = self.orc.triangulate(planes[0], planes[1], P1, P2A)[2]
        pos = z[np.isfinite(z) & (z > 0)]
        return dict(fmt=dn.FMT_16U, unit=60.0 / float(np.percentile(pos, 80)), min_conf=float(np.percentile(planes[2][np.isfinite(planes[2])], 10)))

    def stage_field(self, s):
        """The (dx, dy, conf) field a stage step brings."""
        W, H = s.size
        rng = np.random.Generator(np.random.PCG64(SEED + s.pairs[0]))
        return np.stack([rng.normal(0, 3, (H, W)), rng.normal(0, 1, (H, W)), 0.1 + 0.9 * rng.random((H, W))]).astype(np.float32)

    def key(self, script, i):
        s, st = script[i], settings(script)[i]
        fam = KINDS[s.kind][0]
        cls = _cls(st[0]) if fam not in ("setting",) and s.kind not in ("stage_iterate", "stage_smooth") else None
        lr = st[1] if (lr_on(st) and s.kind in LR_FULL_KINDS) else 0.0
        return (s.kind, s.frame, s.pairs, s.args, cls, lr, self.key(script, s.src) if s.src >= 0 else None)

    def planes_of(self, script, i):
        """The (dx, dy, conf) planes a post-processing step reads: output `out` (pair 0's) of the full-mode step it hangs on."""
        e = self.expected(script, i)
        return e["out"] if "out" in e else e["out0"]

    def expected(self, script, i):
        """{name: array or number} of what step i must leave behind; "status" where the call must be refused."""
        return self._m(("step",) + self.key(script, i), lambda: self._expected(script, i))

    def _expected(self, script, i):
        s, (fmt, tau, _) = script[i], settings(script)[i]
        orc, (W, H), k, fr = self.orc, s.size, s.kind, s.frame
        pairs = pair_of(script, i)
        checked = lr_on(settings(script)[i])                               # the context's full-mode check (ugsm_set_lr_check) is on
        if checked and k in ("full_seeded", "coarse", "fine"):
            return {"status": STATE}                                       # (include/ugsm.h: these calls have no checked form)
        if k in ("full", "full_host"):
            return {"out": self.checked(fr, pairs[0], fmt, tau)[0] if checked else self.full(fr, pairs[0], fmt)}
        if k in ("full_batch", "full_batch_host"):                         # (under the context's check a batch runs pair by pair, every pair checked)
            return {f"out{b}": self.checked(fr, p, fmt, tau)[0] if checked else self.full(fr, p, fmt) for b, p in enumerate(pairs)}
        if k == "full_checked":
            out = {}
            for b, p in enumerate(pairs):
                o, bk, marked = self.checked(fr, p, fmt, s.arg("tau"))
                out.update({f"out{b}": o, f"back{b}": bk, f"marked{b}": marked})
            return out
        if k == "full_seeded":
            L, R = self.seen(fr, pairs[0], fmt)
            return {"out": sn.seeded_oracle(orc, L, R, self.planes_of(script, s.src), s.arg("s"), LEVELS, self.pyr(fr, pairs[0], fmt))}
        if k == "coarse":
            L, R = self.seen(fr, pairs[0], fmt)
            e = s.arg("e")
            state = cs.coarse_oracle(orc, L, R, e, LEVELS, self.pyr(fr, pairs[0], fmt))
            w, h = orc.level_dims(W, H, LEVELS)
            return {"state": state, "full": cs.prolong_np(state, (list(w[:e + 1]), list(h[:e + 1])))}
        if k == "fine":
            L, R = self.seen(fr, pairs[0], fmt)
            return {"out": cs.fine_oracle(orc, L, R, self.expected(script, s.src)["state"], s.arg("e"), LEVELS, self.pyr(fr, pairs[0], fmt))}
        if k in ("fov_batch", "fov_host"):
            out = {}
            for b, p in enumerate(pairs):
                stack, pl, pr = self.fov(fr, p, fmt, s.arg("offsets")[b])
                out[f"stack{b}"] = stack
                if s.arg("pyr"):
                    out.update({f"pyrL{b}": pl, f"pyrR{b}": pr})
            return out
        if k == "fov_multi":
            stacks = [self.fov(fr, pairs[0], fmt, off)[0] for off in s.arg("offsets")]
            out = {f"stack{j}": t for j, t in enumerate(stacks)}
            out["full"] = rm.reconstruct_multi(orc, stacks, W, H, LEVELS, s.arg("offsets"))
            return out
        if k == "fov_multi_checked":
            out = {}
            for j, off in enumerate(s.arg("offsets")):
                chk, counts = self.fov_checked(fr, pairs[0], fmt, off, s.arg("tau"))
                out.update({f"stack{j}": chk, f"marked{j}": counts})
            return out
        if k == "fov_warm":
            L, R = self.seen(fr, pairs[0], fmt)
            prior = self.expected(script, s.src)["stack0"]
            return {"stack0": fs.warm_oracle(orc, L, R, prior, LEVELS, script[s.src].arg("offsets")[0], s.arg("offsets")[0], s.arg("s"), self.pyr(fr, pairs[0], fmt))}
        if k == "fovea_coarse":
            if s.arg("refused"):
                return {"status": STATE}
            L, R = self.seen(fr, pairs[0], fmt)
            return {"state": cs.coarse_oracle(orc, L, R, FOVEA - 1, LEVELS, self.pyr(fr, pairs[0], fmt))}
        if k == "fovea_fine":
            return {"stack0": self.fov(fr, pairs[0], fmt, s.arg("off"))[0]}
        if k == "cloud":
            planes, rgb = self.planes_of(script, s.src), self.seen(fr, pairs[0], fmt)[0]
            return {"cloud": cn.cloud(orc, planes[0], planes[1], rgb, P1, P2A, conf=planes[2], compact=True, **self.cloud_params(planes))}
        if k == "depth16u":
            planes = self.planes_of(script, s.src)
            img, valid = dn.depth_image(orc, planes[0], planes[1], P1, P2A, conf=planes[2], **self.depth_params(planes))
            return {"depth": img, "valid": int(valid.sum())}
        if k in ("warp_right", "residual"):
            planes, (L, R) = self.planes_of(script, s.src), self.seen(fr, pairs[0], fmt)
            Rw = wn.warp(wn.planes(R), planes[0], planes[1])
            if k == "warp_right":
                return {"warp": Rw}
            return {"sums": wn.residual_sums(wn.planes(L), Rw, planes[2]), "quotient": residual_quotient(orc, wn.planes(L), Rw, planes[2])}
        if k == "stage_iterate":
            L, R = self.images(fr, pairs[0])
            mi, S, top, m0, m1 = ITER
            return {"field": orc.iterate_level(orc.rgb_to_planes(L), orc.rgb_to_planes(R), self.stage_field(s), mi, S, bool(top), m0, m1)[0]}
        if k == "stage_smooth":
            d = self.stage_field(s)
            for _ in range(SMOOTH[0]):
                d = orc.smooth_pass(d)
            return {"field": orc.box3(d) if SMOOTH[1] else d}
        if k == "stage_pyramid":
            return {"level": self.pyr(fr, pairs[0], fmt)[0][s.arg("level")]}
        if k == "refused":
            return {"status": {"stride": SIZE_MISMATCH, "small": TOO_SMALL, "empty": BAD_ARG, "nomem": NOMEM}[s.arg("what")]}
        return {}                                                          # pyramids, settings: nothing of their own to compare


# ---- the runner -------------------------------------------------------------------------------------------------------------------------

HOST_GUARD = 1024   # words of poison on either side of a host result buffer


class HostBuf:
    """A host result buffer of n floats between two bands of poison: pageable, or page-locked (ugsm_host_alloc, freed with the context)."""

    def __init__(self, c, n, pinned):
        total = n + 2 * HOST_GUARD
        self.raw = c.host_array((total,), np.uint32) if pinned else np.empty(total, np.uint32)
        self.raw[:] = 0x01010101 * POISON
        self.n = n

    @property
    def floats(self):
        return self.raw[HOST_GUARD:HOST_GUARD + self.n].view(np.float32)

    def planes(self, shape):
        return self.floats.reshape(shape)

    def check(self, what):
        band = np.concatenate([self.raw[:HOST_GUARD], self.raw[HOST_GUARD + self.n:]])
        assert (band == 0x01010101 * POISON).all(), f"{what}: a word outside a host result buffer was written"


class Live:
    """A staged step: its buffers, how it is submitted, and how its outputs are read once its slot has been waited for."""

    def __init__(self, i, s):
        self.i, self.step, self.keep, self.out, self.submit, self.fetch, self.after_wait = i, s, [], {}, None, None, None
        self.images, self.got, self.status = [], {}, None


class Player:
    def __init__(self, lib, c, exp, script, what=""):
        self.lib, self.c, self.exp, self.script, self.what = lib, c, exp, script, what
        self.so, self.h = c.lib, c.handle
        self.set = settings(script)
        self.g = Guards(c)
        self.raw = []          # (pointer, bytes it must still hold, name): images and other byte inputs
        self.poisoned = []     # plain device buffers to free
        self.hosts = []
        self.live = []
        self.bytes = []        # ugsm_context_device_bytes behind every step
        self.dead = False
        self.floats = {}       # floats of every guarded output buffer, by pointer

    # -- buffers
    def dev_bytes(self, arr, name):
        arr = np.ascontiguousarray(arr)
        p = self.c.to_device(arr.view(np.uint8).reshape(-1))
        self.raw.append((p, arr.view(np.uint8).reshape(-1).copy(), name))
        return p

    def image_pair(self, lv, p):
        """The pair in the format in force at the step, rows padded by 8 bytes on odd steps; -> (dL, dR, stride)."""
        i, s = lv.i, lv.step
        fmt = self.set[i][0]
        L, R = self.exp.images(s.frame, p)
        rows = [fl.rows(encode(a, fmt), 8 * (i % 2)) for a in (L, R)]
        dL, dR = (self.dev_bytes(r, f"step {i}: an image") for r in rows)
        lv.images.append((dL, dR, rows[0].shape[1]))
        return dL, dR, rows[0].shape[1]

    def host_pair(self, lv, p, pinned):
        i, s = lv.i, lv.step
        L, R = self.exp.images(s.frame, p)
        rows = [fl.rows(encode(a, self.set[i][0]), 8) for a in (L, R)]
        if pinned:
            held = []
            for r in rows:
                a = self.c.host_array(r.shape, np.uint8)
                a[:] = r
                held.append(a)
            rows = held
        lv.keep.append((rows, [r.copy() for r in rows]))
        return rows[0], rows[1], rows[0].shape[1]

    def fbuf(self, n, shift=0):
        p = self.g.buf(n, shift)
        self.floats[p] = n
        return p

    def untouched(self, lv):
        """Every device output of a refused step, as it stands: the poison it was filled with."""
        raw = [self.g.check(p, (self.floats[p],), f"step {lv.i} {name}") for name, p in lv.out.items() if p in self.floats]
        return {"untouched": np.concatenate(raw) if raw else np.empty(0, np.float32)}

    def hbuf(self, n, pinned):
        b = HostBuf(self.c, n, pinned)
        self.hosts.append(b)
        return b

    def poison(self, nbytes):
        p = self.c.to_device(np.full(nbytes, POISON, np.uint8))
        self.poisoned.append(p)
        return p

    def read_poisoned(self, p, nbytes, used, name):
        raw = self.c.to_host(p, (nbytes,), np.uint8)
        assert (raw[used:] == POISON).all(), f"{name}: a byte past what the call writes was touched"
        return raw[:used]

    def src_planes(self, s):
        """Device pointers of the (dx, dy, conf) planes of the step `s` hangs on."""
        src = self.live[s.src]
        W, H = src.step.size
        base = src.out["out"] if "out" in src.out else src.out["out0"]
        return base, base + 4 * W * H, base + 8 * W * H

    # -- staging, kind by kind: fills lv.out (device pointers by output name), lv.submit, lv.fetch
    def stage(self, i):
        s = self.script[i]
        lv = Live(i, s)
        self.live.append(lv)
        getattr(self, "_" + s.kind)(lv, s)
        return lv

    def _planes_fetch(self, lv, shapes):
        def fetch():
            return {name: self.g.check(lv.out[name], shape, f"step {lv.i} {name}") for name, shape in shapes.items()}
        lv.fetch = fetch

    def _full(self, lv, s):
        W, H = s.size
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        lv.out["out"] = self.fbuf(3 * W * H, lv.i % 4)
        lv.submit = lambda: self.so.ugsm_submit_full(self.h, s.slot, dL, dR, W, H, stride, lv.out["out"])
        self._planes_fetch(lv, {"out": (3, H, W)})
        self._marked(lv, s)

    def _marked(self, lv, s):
        """ugsm_last_lr_marked behind a single-pair call, read when the call is still the slot's last: the oracle's count under the context's
        check, -1 without it."""
        fmt, tau, _ = self.set[lv.i]
        lv.after_wait = lambda: {"last_lr_marked": self.c.last_lr_marked(s.slot)}
        lv.want_marked = self.exp.checked(s.frame, s.pairs[0], fmt, tau)[2][0] if lr_on(self.set[lv.i]) else -1

    def _full_batch(self, lv, s):
        W, H = s.size
        imgs = [self.image_pair(lv, p) for p in s.pairs]
        for b in range(s.n):
            lv.out[f"out{b}"] = self.fbuf(3 * W * H, (lv.i + b) % 4)
        ptr = self.c._ptrs
        lv.submit = lambda: self.so.ugsm_submit_full_batch(self.h, s.slot, s.n, ptr([m[0] for m in imgs]), ptr([m[1] for m in imgs]), W, H, imgs[0][2],
                                                           ptr([lv.out[f"out{b}"] for b in range(s.n)]))
        self._planes_fetch(lv, {f"out{b}": (3, H, W) for b in range(s.n)})

    def _full_host(self, lv, s):
        W, H = s.size
        L, R, stride = self.host_pair(lv, s.pairs[0], False)
        o = self.hbuf(3 * W * H, False)
        pl = o.planes((3, H, W))
        lv.submit = lambda: self.so.ugsm_match_full(self.h, L.ctypes.data, R.ctypes.data, W, H, stride, *[pl[k].ctypes.data for k in range(3)])
        lv.fetch = lambda: {"out": pl.copy()}
        self._marked(lv, s)

    def _full_batch_host(self, lv, s):
        W, H = s.size
        imgs = [self.host_pair(lv, p, True) for p in s.pairs]
        outs = [self.hbuf(3 * W * H, True).planes((3, H, W)) for _ in s.pairs]
        lv.submit = lambda: self.so.ugsm_submit_full_batch_host(
            self.h, s.slot, s.n, self.c._ptrs([m[0].ctypes.data for m in imgs]), self.c._ptrs([m[1].ctypes.data for m in imgs]), W, H, imgs[0][2],
            *[self.c._ptrs([o[k].ctypes.data for o in outs]) for k in range(3)])
        lv.fetch = lambda: {f"out{b}": o.copy() for b, o in enumerate(outs)}

    def _full_checked(self, lv, s):
        W, H = s.size
        imgs = [self.image_pair(lv, p) for p in s.pairs]
        for b in range(s.n):
            lv.out[f"out{b}"], lv.out[f"back{b}"] = self.fbuf(3 * W * H), self.fbuf(3 * W * H)
        ptr = self.c._ptrs
        lv.submit = lambda: self.so.ugsm_submit_full_checked(self.h, s.slot, s.n, ptr([m[0] for m in imgs]), ptr([m[1] for m in imgs]), W, H, imgs[0][2],
                                                             ptr([lv.out[f"out{b}"] for b in range(s.n)]), ptr([lv.out[f"back{b}"] for b in range(s.n)]),
                                                             C.c_float(s.arg("tau")))
        self._planes_fetch(lv, {name: (3, H, W) for name in lv.out})
        lv.after_wait = lambda: {f"marked{b}": self.c.last_lr_marked_pair(s.slot, b) for b in range(s.n)}

    def _full_seeded(self, lv, s):
        W, H = s.size
        dL, dR, stride = self.image_pair(lv, pair_of(self.script, lv.i)[0])
        prior = self.src_planes(s)[0]
        lv.out["out"] = self.fbuf(3 * W * H, lv.i % 4)
        one = lambda p: self.c._ptrs([p])
        lv.submit = lambda: self.so.ugsm_submit_full_seeded(self.h, s.slot, 1, one(dL), one(dR), W, H, stride, one(prior), s.arg("s"), one(lv.out["out"]))
        self._planes_fetch(lv, {"out": (3, H, W)})

    def _coarse(self, lv, s):
        W, H = s.size
        w, h = self.lib.level_dims(W, H, LEVELS)
        e = s.arg("e")
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        lv.out["state"], lv.out["full"] = self.fbuf(3 * w[e] * h[e]), self.fbuf(3 * W * H, lv.i % 4)
        one = lambda p: self.c._ptrs([p])
        lv.submit = lambda: self.so.ugsm_submit_full_coarse(self.h, s.slot, 1, one(dL), one(dR), W, H, stride, e, one(lv.out["state"]), one(lv.out["full"]))
        self._planes_fetch(lv, {"state": (3, h[e], w[e]), "full": (3, H, W)})

    def _fine(self, lv, s):
        W, H = s.size
        dL, dR, stride = self.image_pair(lv, pair_of(self.script, lv.i)[0])
        state = self.live[s.src].out["state"]
        lv.out["out"] = self.fbuf(3 * W * H, lv.i % 4)
        one = lambda p: self.c._ptrs([p])
        lv.submit = lambda: self.so.ugsm_submit_full_fine(self.h, s.slot, 1, one(dL), one(dR), W, H, stride, one(state), s.arg("e"), one(lv.out["out"]))
        self._planes_fetch(lv, {"out": (3, H, W)})

    def _stack_dims(self, s):
        fw, fh = self.lib.fovea_dims(*s.size, LEVELS, FOVEA)
        return fw, fh, 3 * FOVEA * fw * fh

    def _fov_batch(self, lv, s):
        W, H = s.size
        fw, fh, n3 = self._stack_dims(s)
        imgs = [self.image_pair(lv, p) for p in s.pairs]
        shapes = {}
        for b in range(s.n):
            lv.out[f"stack{b}"] = self.fbuf(n3)
            shapes[f"stack{b}"] = (3, FOVEA, fh, fw)
            if s.arg("pyr"):
                lv.out[f"pyrL{b}"], lv.out[f"pyrR{b}"] = self.fbuf(n3), self.fbuf(n3)
                shapes[f"pyrL{b}"] = shapes[f"pyrR{b}"] = (FOVEA, 3, fh, fw)
        ptr = self.c._ptrs
        ox, oy = self.c._offsets(s.arg("offsets"), s.n)
        pyr = [ptr([lv.out[f"pyr{side}{b}"] for b in range(s.n)]) if s.arg("pyr") else None for side in "LR"]
        lv.submit = lambda: self.so.ugsm_submit_foveated_batch(self.h, s.slot, s.n, ptr([m[0] for m in imgs]), ptr([m[1] for m in imgs]), W, H, imgs[0][2],
                                                               ox, oy, ptr([lv.out[f"stack{b}"] for b in range(s.n)]), pyr[0], pyr[1])
        self._planes_fetch(lv, shapes)

    def _fov_host(self, lv, s):
        W, H = s.size
        fw, fh, n3 = self._stack_dims(s)
        L, R, stride = self.host_pair(lv, s.pairs[0], False)
        st = self.hbuf(n3, False).planes((3, FOVEA, fh, fw))
        pyr = [self.hbuf(n3, False).planes((FOVEA, 3, fh, fw)) for _ in range(2)] if s.arg("pyr") else [None, None]
        off = s.arg("offsets")[0]
        lv.submit = lambda: self.so.ugsm_match_foveated(self.h, L.ctypes.data, R.ctypes.data, W, H, stride, off[0], off[1], *[st[k].ctypes.data for k in range(3)],
                                                        *[p.ctypes.data if p is not None else None for p in pyr])
        lv.fetch = lambda: {"stack0": st.copy(), **({"pyrL0": pyr[0].copy(), "pyrR0": pyr[1].copy()} if s.arg("pyr") else {})}

    def _fov_multi(self, lv, s, tau=None):
        W, H = s.size
        fw, fh, n3 = self._stack_dims(s)
        offs = s.arg("offsets")
        n = len(offs)
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        shapes = {}
        for j in range(n):
            lv.out[f"stack{j}"] = self.fbuf(n3)
            shapes[f"stack{j}"] = (3, FOVEA, fh, fw)
        ox, oy = self.c._offsets(offs, n)
        stacks = self.c._ptrs([lv.out[f"stack{j}"] for j in range(n)])
        if tau is None:
            lv.out["full"] = self.fbuf(3 * W * H, lv.i % 4)
            shapes["full"] = (3, H, W)

            def submit():
                st = self.so.ugsm_submit_foveated_multi(self.h, s.slot, dL, dR, W, H, stride, n, ox, oy, stacks)
                return st or self.so.ugsm_reconstruct_full_multi(self.h, s.slot, n, stacks, W, H, ox, oy, lv.out["full"])
            lv.submit = submit
        else:
            lv.submit = lambda: self.so.ugsm_submit_foveated_multi_checked(self.h, s.slot, dL, dR, W, H, stride, n, ox, oy, stacks, C.c_float(tau))
            lv.after_wait = lambda: {f"marked{j}": self.c.last_lr_marked_levels(s.slot, j) for j in range(n)}
        self._planes_fetch(lv, shapes)

    def _fov_multi_checked(self, lv, s):
        self._fov_multi(lv, s, s.arg("tau"))

    def _fov_warm(self, lv, s):
        W, H = s.size
        fw, fh, n3 = self._stack_dims(s)
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        prior, poff, off = self.live[s.src].out["stack0"], self.script[s.src].arg("offsets")[:1], s.arg("offsets")
        lv.out["stack0"] = self.fbuf(n3)
        one = lambda p: self.c._ptrs([p])
        ox, oy = self.c._offsets(off, 1)
        px, py = self.c._offsets(poff, 1)
        lv.submit = lambda: self.so.ugsm_submit_foveated_warm(self.h, s.slot, 1, one(dL), one(dR), W, H, stride, ox, oy, one(prior), px, py, s.arg("s"),
                                                              one(lv.out["stack0"]))
        self._planes_fetch(lv, {"stack0": (3, FOVEA, fh, fw)})

    def _pyramids(self, lv, s):
        W, H = s.size
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        lv.submit = lambda: self.so.ugsm_submit_pyramids(self.h, s.slot, dL, dR, W, H, stride)
        lv.fetch = lambda: {}

    def _fovea_coarse(self, lv, s):
        fw, fh, _ = self._stack_dims(s)
        lv.out["state"] = self.fbuf(3 * fw * fh)
        lv.submit = lambda: self.so.ugsm_submit_fovea_coarse(self.h, s.slot, lv.out["state"])
        self._planes_fetch(lv, {"state": (3, fh, fw)})

    def _fovea_fine(self, lv, s):
        fw, fh, n3 = self._stack_dims(s)
        state, off = self.live[s.src].out["state"], s.arg("off")
        lv.out["stack0"] = self.fbuf(n3)
        lv.submit = lambda: self.so.ugsm_submit_fovea_fine(self.h, s.slot, state, off[0], off[1], lv.out["stack0"])
        self._planes_fetch(lv, {"stack0": (3, FOVEA, fh, fw)})

    def _proj(self, lv, P_):
        dp = C.POINTER(C.c_double)
        arrs = [np.ascontiguousarray(P, np.float64).reshape(12) for P in (P1, P_)]
        lv.keep.append(arrs)
        return [a.ctypes.data_as(dp) for a in arrs]

    def _cloud(self, lv, s):
        W, H = s.size
        dL, _, stride = self.image_pair(lv, pair_of(self.script, lv.i)[0])
        dx, dy, conf = self.src_planes(s)
        prm = self.lib.cloud_params(compact=True, **self.exp.cloud_params(self.exp.planes_of(self.script, s.src)))
        cap, item = cn.cloud_points(W, H, 1), cn.DTYPES[cn.PCL32].itemsize
        pts, cnt = self.poison((cap + EXTRA) * item), self.c.to_device(np.full(1, -7, np.int64))
        self.poisoned.append(cnt)
        q1, q2 = self._proj(lv, P2A)
        lv.keep.append(prm)
        lv.submit = lambda: self.so.ugsm_point_cloud(self.h, s.slot, dx, dy, conf, dL, W, H, stride, q1, q2, C.byref(prm), pts, cap, cnt)

        def fetch():
            count = int(self.c.to_host(cnt, (1,), np.int64)[0])
            assert 0 <= count <= cap, f"step {lv.i}: the cloud's count is {count}"
            return {"cloud": self.read_poisoned(pts, (cap + EXTRA) * item, count * item, f"step {lv.i} cloud").view(cn.DTYPES[cn.PCL32])}
        lv.fetch = fetch

    def _depth16u(self, lv, s):
        W, H = s.size
        dx, dy, conf = self.src_planes(s)
        kw = dict(self.exp.depth_params(self.exp.planes_of(self.script, s.src)))
        prm = self.lib.depth_params(format=kw.pop("fmt"), **kw)
        img, valid = self.poison(2 * (W * H + EXTRA)), self.poison(8 + EXTRA)
        q1, q2 = self._proj(lv, P2A)
        lv.keep.append(prm)
        lv.submit = lambda: self.so.ugsm_depth_image(self.h, s.slot, dx, dy, conf, W, H, q1, q2, C.byref(prm), img, valid)
        lv.fetch = lambda: {"depth": self.read_poisoned(img, 2 * (W * H + EXTRA), 2 * W * H, f"step {lv.i} depth").view(np.uint16).reshape(H, W),
                            "valid": int(self.read_poisoned(valid, 8 + EXTRA, 8, f"step {lv.i} valid").view(np.uint64)[0])}

    def _warp_right(self, lv, s):
        W, H = s.size
        _, dR, stride = self.image_pair(lv, pair_of(self.script, lv.i)[0])
        dx, dy, _ = self.src_planes(s)
        lv.out["warp"] = self.fbuf(3 * W * H, lv.i % 4)
        lv.submit = lambda: self.so.ugsm_warp_right(self.h, s.slot, dR, W, H, stride, dx, dy, lv.out["warp"])
        self._planes_fetch(lv, {"warp": (3, H, W)})

    def _residual(self, lv, s):
        W, H = s.size
        dL, dR, stride = self.image_pair(lv, pair_of(self.script, lv.i)[0])
        dx, dy, conf = self.src_planes(s)
        sums = self.poison(32 + EXTRA)
        lv.submit = lambda: self.so.ugsm_photometric_residual(self.h, s.slot, dL, dR, W, H, stride, dx, dy, conf, sums)

        def fetch():
            raw = self.read_poisoned(sums, 32 + EXTRA, 32, f"step {lv.i} sums").view(np.float64).copy()
            with np.errstate(all="ignore"):
                return {"sums": raw, "quotient": (raw[:3] / raw[3]).astype(np.float32)}
        lv.fetch = fetch

    def _stage_iterate(self, lv, s):
        W, H = s.size
        orc = self.exp.orc
        L, R = self.exp.images(s.frame, s.pairs[0])
        pL, pR = self.g.inp(orc.rgb_to_planes(L), 0), self.g.inp(orc.rgb_to_planes(R), 0)
        lv.out["field"] = self.g.buf(3 * W * H, 0, self.exp.stage_field(s))
        mi, S, top, m0, m1 = ITER
        lv.submit = lambda: self.so.ugsm_stage_iterate(self.h, pL, pR, lv.out["field"], W, H, mi, S, top, m0, m1, None)
        self._planes_fetch(lv, {"field": (3, H, W)})

    def _stage_smooth(self, lv, s):
        W, H = s.size
        lv.out["field"] = self.g.buf(3 * W * H, 0, self.exp.stage_field(s))
        lv.submit = lambda: self.so.ugsm_stage_smooth(self.h, lv.out["field"], W, H, *SMOOTH)
        self._planes_fetch(lv, {"field": (3, H, W)})

    def _stage_pyramid(self, lv, s):
        W, H = s.size
        w, h = self.lib.level_dims(W, H, LEVELS)
        lev = s.arg("level")
        dL, _, stride = self.image_pair(lv, s.pairs[0])
        lv.out["level"] = self.fbuf(3 * w[lev] * h[lev])
        lv.submit = lambda: self.so.ugsm_stage_pyramid(self.h, dL, W, H, stride, lev, lv.out["level"])
        self._planes_fetch(lv, {"level": (3, h[lev], w[lev])})

    def _set_format(self, lv, s):
        lv.submit = lambda: self.so.ugsm_set_input_format(self.h, s.arg("fmt"))
        lv.fetch = lambda: {}

    def _set_lr(self, lv, s):
        lv.submit = lambda: self.so.ugsm_set_lr_check(self.h, C.c_float(s.arg("tau")), s.arg("modes"))
        lv.fetch = lambda: {}

    def _refused(self, lv, s):
        """A ugsm_submit_full that must be refused before anything is enqueued: rows one byte short; a frame with no pyramid of the context's
        levels (11 x 9: too small; 0 x H: no frame at all); `nomem`: a batch the context's memory limit does not hold."""
        W, H = s.size
        what = s.arg("what")
        if what == "nomem":
            return self._refused_nomem(lv, s)
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        bpp = self.lib.INPUT_BYTES_PER_PIXEL[self.set[lv.i][0]]
        w_, h_, st_ = {"stride": (W, H, bpp * W - 1), "small": (11, 9, stride), "empty": (0, H, stride)}[what]
        lv.out["out"] = self.fbuf(3 * W * H)
        lv.submit = lambda: self.so.ugsm_submit_full(self.h, s.slot, dL, dR, w_, h_, st_, lv.out["out"])
        self._planes_fetch(lv, {"out": (3, H, W)})

    def _refused_nomem(self, lv, s):
        W, H = s.size
        n = s.arg("n")
        dL, dR, stride = self.image_pair(lv, s.pairs[0])
        lv.out["out"] = self.fbuf(3 * W * H)
        ptr = self.c._ptrs
        lv.submit = lambda: self.so.ugsm_submit_full_batch(self.h, s.slot, n, ptr([dL] * n), ptr([dR] * n), W, H, stride, ptr([lv.out["out"]] * n))
        self._planes_fetch(lv, {"out": (3, H, W)})

    # -- the pass
    def wait(self, slot):
        self.c.check(self.so.ugsm_wait(self.h, slot))

    def run(self):
        """Stages everything, submits the calls back to back, waits once per slot; returns the Live records with .got filled."""
        for i in range(len(self.script)):
            self.stage(i)
        last = {}
        for lv in self.live:
            s = lv.step
            lv.status = int(lv.submit())
            want = self.exp.expected(self.script, lv.i).get("status", OK)
            assert lv.status == want, (f"{self.what}step {lv.i} ({s}): status {lv.status} ({self.lib.status_string(lv.status)}: "
                                       f"{self.so.ugsm_last_error(self.h).decode()}), expected {want}")
            self.bytes.append(self.c.device_bytes())
            if lv.status != OK:                                          # refused, as expected: nothing was written
                lv.fetch = lambda lv=lv: self.untouched(lv)
            if s.arg("direct") is not None:                              # (development library: which way the call read level 0)
                took = self.so.ugsm_stage_level0_direct(self.h, s.slot)
                assert took == s.arg("direct"), f"{self.what}step {lv.i} ({s}): ugsm_stage_level0_direct {took}, expected {s.arg('direct')}"
            if KINDS[s.kind][0] == "setting":
                continue
            last[s.slot] = lv
            if s.wait_after:
                self.wait(s.slot)
                if lv.after_wait and lv.status == OK:
                    lv.got.update(lv.after_wait())
        for slot in sorted(last):
            self.wait(slot)
            lv = last[slot]
            if lv.after_wait and lv.status == OK and not lv.step.wait_after:
                lv.got.update(lv.after_wait())
        for lv in self.live:
            lv.got.update(lv.fetch())
        return self.live

    def inputs_untouched(self):
        for p, sent, name in self.raw:
            back = self.c.to_host(p, (sent.size,), np.uint8)
            assert np.array_equal(back, sent), f"{self.what}{name} was written"
        for lv in self.live:
            for rows, sent in (k for k in lv.keep if isinstance(k, tuple)):
                for a, b in zip(rows, sent):
                    assert np.array_equal(a, b), f"{self.what}step {lv.i}: a host image was written"
        for b in self.hosts:
            b.check(self.what)

    def close(self):
        """Guards.done (every buffer not read back, the inputs' contents) and every buffer of the pass freed; for a `finally`."""
        if self.dead:
            return
        try:
            self.g.done(self.what)
        finally:
            for p, _, _ in self.raw:
                self.c.free(p)
            for p in self.poisoned:
                self.c.free(p)
            self.raw, self.poisoned = [], []


def compare(name, got, exp, what):
    if name == "untouched":
        assert (np.asarray(got).view(np.uint8) == POISON).all(), f"{what}: a refused call wrote to its output"
    elif name == "cloud":
        assert got.size == exp.size, f"{what}: {got.size} records, expected {exp.size}"
        cn.assert_cloud_equal(got, exp, what)
    elif name == "depth":
        dn.assert_image_equal(got, exp, what)
    elif name == "sums":
        assert got.tobytes() == exp.tobytes(), f"{what}: the raw sums {got} vs {exp}"
    elif isinstance(exp, np.ndarray):
        assert_bit_equal(got, exp, what)
    else:
        assert (list(got) if isinstance(got, (list, tuple)) else got) == (list(exp) if isinstance(exp, (list, tuple)) else exp), f"{what}: {got} vs {exp}"


def check_step(exp, script, lv, what=""):
    """Every output of the step against its expected value; a refused step leaves its poison."""
    e = exp.expected(script, lv.i)
    where = f"{what}step {lv.i} ({lv.step})"
    for name, want in e.items():
        if name == "status":
            continue
        assert name in lv.got or name.startswith("marked"), f"{where}: output {name} was not read back"
        if name in lv.got:
            compare(name, lv.got[name], want, f"{where} {name}")
    if "untouched" in lv.got:
        compare("untouched", lv.got["untouched"], None, where)
    if "last_lr_marked" in lv.got:
        assert lv.got["last_lr_marked"] == lv.want_marked, f"{where}: ugsm_last_lr_marked {lv.got['last_lr_marked']}, expected {lv.want_marked}"
    for name in lv.got:
        assert name in e or name in ("untouched", "last_lr_marked"), f"{where}: output {name} has no expected value"


def chain(script, i):
    """The steps step i needs when it is played alone: the steps it hangs on, in order, every one waited for, under the settings it captures."""
    need, j = [], i
    while j >= 0:
        need.append(j)
        j = script[j].src
    need.reverse()
    fmt, tau, modes = settings(script)[i]
    pre = ([step("set_format", fmt=fmt)] if fmt != RGB8 else []) + ([step("set_lr", tau=tau, modes=modes)] if tau > 0 else [])
    new = {j: len(pre) + k for k, j in enumerate(need)}
    return pre + [Step(script[j].kind, script[j].frame, script[j].pairs, script[j].args, script[j].slot, True, new.get(script[j].src, -1)) for j in need]


def diagnose(lib, cfg, exp, script, i):
    """Step i alone on a fresh context: "state" if it is right there (an earlier call left the slot wrong for it), "kernel" if it is wrong there too."""
    alone = chain(script, i)
    with lib.Context(**cfg) as c:
        p = Player(lib, c, exp, alone, "alone on a fresh context: ")
        try:
            live = p.run()
            check_step(exp, alone, live[-1], "alone on a fresh context: ")
            return "state"
        except AssertionError:
            return "kernel"
        finally:
            p.g.free()
            p.close()


def play(lib, c, exp, script, cfg=None, what=""):
    """One pass of the script on the context; returns ugsm_context_device_bytes behind every step.  Every step's outputs are compared (the
    first mismatch raises, after the failing step has been played alone on a fresh context where `cfg` is given), then guards and inputs."""
    p = Player(lib, c, exp, script, what)
    try:
        live = p.run()
        for lv in live:
            try:
                check_step(exp, script, lv, what)
            except AssertionError as e:
                before = [j for j in range(lv.i) if script[j].slot == lv.step.slot and KINDS[script[j].kind][0] != "setting"]
                prev = f"step {before[-1]} ({script[before[-1]]})" if before else "nothing"
                verdict = diagnose(lib, cfg, exp, script, lv.i) if cfg is not None else None
                note = {"state": "played alone on a fresh context the step is RIGHT: a state bug -- what an earlier call left in the slot",
                        "kernel": "played alone on a fresh context the step is WRONG too: the step itself, not the slot's history", None: ""}[verdict]
                raise AssertionError(f"{e}\n  before it on slot {lv.step.slot}: {prev}\n  {note}") from e
        p.inputs_untouched()
        return p.bytes
    except lib.UgsmError:
        p.dead = True          # (a call or a copy failed on the device: nothing more is read back or compared on it)
        raise
    finally:
        p.close()


def play_twice(lib, cfg, exp, script, what=""):
    """The script on a fresh context, then once more on the same, now warm, context.  Returns (bytes after the first pass, after the replay):
    during the first pass ugsm_context_device_bytes never decreases, and the replay allocates nothing."""
    with lib.Context(**cfg) as c:
        first = play(lib, c, exp, script, cfg, what + "first pass: ")
        assert all(b >= a for a, b in zip(first, first[1:])), f"{what}device bytes decreased during the first pass: {first}"
        again = play(lib, c, exp, script, cfg, what + "replay: ")
        print(f"{what}device bytes after the first pass {first[-1]}, after the replay {again[-1]}")
        assert set(again) == {first[-1]}, f"{what}the warm context allocated: {first[-1]} after the first pass, {again} during the replay"
        return first[-1], again[-1]


# ---- the random walks --------------------------------------------------------------------------------------------------------------------

WALK_FRAMES = ("A", "B", "T", "Wd")
WALK_MOVES = 40


def walk(seed):
    """A script of WALK_MOVES moves on the main context, a plain function of the seed.  A move is a call, or a call with what hangs on it (a
    seeded call with the full call it starts from, the two halves, the fovea phases behind their pyramids, the post-processing of a match):
    every kind at least twice does not fit into 40 single calls.  Frames from A, B, T, Wd; both slots; a call is waited for with probability
    1/3; a format or LR setting is put back a few moves later, and at the end."""
    rng = np.random.Generator(np.random.PCG64(seed))
    script, state = [], {"pair": 1000 * (seed % 1000), "fmt": RGB8, "lr": 0.0}

    def pair():
        state["pair"] += 1
        return state["pair"]

    def common(blocking=False):
        return dict(frame=WALK_FRAMES[int(rng.integers(len(WALK_FRAMES)))], slot=0 if blocking else int(rng.integers(2)), wait=bool(rng.random() < 1 / 3))

    def offs(n):
        return tuple((int(rng.integers(-60, 61)), int(rng.integers(-40, 41))) for _ in range(n))

    def add(kind, kw, n=1, src=-1, **args):
        script.append(step(kind, kw["frame"], [pair() for _ in range(n)], kw["slot"], kw["wait"], src, **args))
        return len(script) - 1

    moves = {
        "full": lambda kw: add("full", kw),
        "full_batch": lambda kw: add("full_batch", kw, int(rng.integers(2, 4))),
        "full_host": lambda kw: add("full_host", kw),
        "full_batch_host": lambda kw: add("full_batch_host", kw, 2),
        "full_checked": lambda kw: (add("full_checked", {**kw, "wait": False}, int(rng.integers(1, 3)), tau=TAU), add("full", kw)),
        "seeded": lambda kw: add("full_seeded", kw, 1, add("full", kw), s=int(rng.integers(1, 4))),
        "halves": lambda kw: (lambda e: add("fine", kw, 0, add("coarse", kw, e=e), e=e))(int(rng.integers(1, 5))),
        "fov_batch": lambda kw: (lambda n: add("fov_batch", kw, n, offsets=offs(n), pyr=bool(rng.integers(2))))(int(rng.integers(1, 3))),
        "fov_host": lambda kw: add("fov_host", kw, offsets=offs(1), pyr=bool(rng.integers(2))),
        "fov_multi": lambda kw: add("fov_multi", kw, offsets=offs(3)),
        "fov_multi_checked": lambda kw: add("fov_multi_checked", kw, offsets=offs(2), tau=TAU),
        "warm": lambda kw: add("fov_warm", kw, 1, add("fov_batch", kw, 1, offsets=offs(1), pyr=False), offsets=offs(1), s=int(rng.integers(0, FOVEA))),
        "phases": lambda kw: add("fovea_fine", kw, 0, add("fovea_coarse", kw, 0, add("pyramids", kw)), off=offs(1)[0]),
        "post": lambda kw: (lambda f: [add(k, kw, 0, f) for k in ("cloud", "depth16u", "warp_right", "residual")])(add("full", kw)),
        "stage_iterate": lambda kw: add("stage_iterate", kw),
        "stage_smooth": lambda kw: add("stage_smooth", kw),
        "stage_pyramid": lambda kw: add("stage_pyramid", kw, level=int(rng.integers(0, 4))),
        "refused": lambda kw: [add("refused", kw, what=w) for w in ("stride", "small", "empty")],
    }
    blocking = {"full_host", "fov_host", "stage_iterate", "stage_smooth", "stage_pyramid"}
    names = sorted(moves)
    order = list(rng.permutation(names * 2))                         # every move twice ...
    restore = {}                                                     # move number -> the settings put back there

    def behind_unwaited():
        """The call submitted last is not waited for (where it can be: not a blocking one): the setting changes right behind it."""
        if script and not KINDS[script[-1].kind][2] and KINDS[script[-1].kind][0] != "setting":
            p = script[-1]
            script[-1] = Step(p.kind, p.frame, p.pairs, p.args, p.slot, False, p.src)

    for m in range(WALK_MOVES):
        for what in restore.pop(m, ()):
            script.append(step("set_format", fmt=RGB8) if what == "fmt" else step("set_lr", tau=0.0, modes=0))
        if m in (5, 17, 29):                                         # ... and the settings in between, right behind whatever was submitted last
            behind_unwaited()
            script.append(step("set_format", fmt=(BGR8, MONO8, RGB32F)[(m // 12 + seed) % 3]))
            restore.setdefault(m + 3, []).append("fmt")
        if m in (9, 23):
            behind_unwaited()
            script.append(step("set_lr", tau=TAU, modes=1))
            restore.setdefault(m + 4, []).append("lr")
        name = order[m] if m < len(order) else names[int(rng.integers(len(names)))]
        moves[name](common(name in blocking))
    for what in sorted({w for v in restore.values() for w in v}):
        script.append(step("set_format", fmt=RGB8) if what == "fmt" else step("set_lr", tau=0.0, modes=0))
    return script


# ---- the scripted groups -----------------------------------------------------------------------------------------------------------------
# name -> (script, what the script is there for: the transitions that test_context_life_host.py finds in it, by slot).  Every step of a group
# brings pairs of its own: no two expected arrays of a script are the same image's.

OFFS3 = ((0, 0), (-60, 30), (50, -40))
DIRECT = dict(march_min_pixels=1)            # with UGSM_MARCH4=0,0: every level through k_cost_march, level 0 read from rgb8 images (test_gpu_level0_direct.py)


def _post(script, src, wait_last=False):
    for k, kind in enumerate(("cloud", "depth16u", "warp_right", "residual")):
        script.append(step(kind, script[src].frame, src=src, wait=wait_last and k == 3))


def group_a():
    """Grow, reuse, shrink, grow: C right behind an unwaited A (the slot's buffers, sized for the context's batch of A frames, are freed and
    regrown under the running call); A again on the warm slot; three B, tall, flat; two C."""
    return [step("full", "A", 101, wait=False), step("full", "C", 102), step("full", "A", 103, wait=False),
            step("full_batch", "B", (104, 105, 106), wait=False), step("full", "T", 107, wait=False), step("full", "Wd", 108, wait=False),
            step("full_batch", "C", (109, 110))]


def group_b():
    """The batch dimension on one slot with no waits: 3, 1, 2 pairs; a checked call of two (four entries) and a plain one right behind it; a
    checked call whose counts are read, and a plain one."""
    return [step("full_batch", "B", (201, 202, 203), wait=False), step("full", "B", 204, wait=False), step("full_batch", "B", (205, 206), wait=False),
            step("full_checked", "B", (207, 208), wait=False, tau=TAU), step("full", "B", 209), step("full_checked", "B", (210,), tau=TAU),
            step("full", "B", 211)]


def group_c():
    """Staging layouts on slot 0: three windows, the blocking full and foveated host calls, a foveated batch with pyramid stacks, a
    page-locked batch, the checked windows."""
    return [step("fov_multi", "B", 301, wait=False, offsets=OFFS3), step("full_host", "B", 302), step("fov_host", "A", 303, offsets=((20, -10),), pyr=True),
            step("fov_batch", "B", (304, 305), wait=False, offsets=((0, 0), (-45, 25)), pyr=True), step("full_batch_host", "A", (306, 307), wait=False),
            step("fov_multi_checked", "B", 308, offsets=OFFS3[:2], tau=TAU)]


def group_d():
    """What a call leaves behind (a context of DIRECT: a full-mode call stores no level 0): the fovea phases refused behind a full call, served
    behind ugsm_submit_pyramids -- three refused calls in between change nothing --, refused again behind a stage call; then a seeded call,
    the two halves, a warm foveated call from a window stack."""
    s = [step("full", "B", 401), step("fovea_coarse", "B", refused=True), step("pyramids", "B", 402, wait=False)]
    s += [step("refused", "B", 403 + k, what=w) for k, w in enumerate(("stride", "small", "empty"))]
    s += [step("fovea_coarse", "B", src=2, wait=False), step("fovea_fine", "B", src=6, off=(21, -13)), step("stage_iterate", "A", 406),
          step("fovea_coarse", "B", refused=True), step("full", "B", 407, wait=False), step("full_seeded", "B", 408, src=10, wait=False, s=2),
          step("coarse", "B", 409, wait=False, e=3), step("fine", "B", src=12, wait=False, e=3), step("fov_multi", "B", 410, wait=False, offsets=OFFS3),
          step("fov_warm", "B", 411, src=14, offsets=((15, 10),), s=1)]
    return s


def group_e():
    """Settings right behind an unfinished call: bgr8, mono8, rgb32f and back; the LR check on and off."""
    return [step("full", "B", 501, wait=False), step("set_format", fmt=BGR8), step("full", "B", 502, wait=False), step("set_format", fmt=MONO8),
            step("full", "A", 503, wait=False), step("set_format", fmt=RGB32F), step("full", "A", 504, wait=False), step("set_format", fmt=RGB8),
            step("full", "B", 505, wait=False), step("set_lr", tau=TAU, modes=1), step("full", "B", 506), step("set_lr", tau=0.0, modes=0),
            step("full", "A", 507)]


def group_f():
    """Level 0 read from the images, then everything else (DIRECT, development library): direct, not direct in bgr8, a foveated batch, direct
    at another size, the fovea phases, a checked call."""
    return [step("full", "B", 601, wait=False, direct=1), step("set_format", fmt=BGR8), step("full", "B", 602, wait=False, direct=0),
            step("set_format", fmt=RGB8), step("fov_batch", "B", (603, 604), wait=False, offsets=((0, 0), (30, 20)), pyr=False),
            step("full", "A", 605, wait=False, direct=1), step("pyramids", "A", 606, wait=False), step("fovea_coarse", "A", src=6, wait=False),
            step("fovea_fine", "A", src=7, wait=False, off=(-12, 9)), step("full_checked", "B", (607,), tau=TAU)]


def group_g():
    """Post-processing between matches: cloud, depth image, warped right image and residual on B's planes, on A's, on B's again -- the count
    buffer and the residual's rows see a larger, a smaller and a larger frame."""
    s = [step("full", "B", 701, wait=False)]
    _post(s, 0)
    s.append(step("full", "A", 702, wait=False))
    _post(s, 5)
    s.append(step("full", "B", 703, wait=False))
    _post(s, 10, wait_last=True)
    return s


def group_h(third_slot=False):
    """Two slots: slot 1 alone borrows slot 0's stream; at once three pairs on slot 0; windows on slot 1 and a C on slot 0 that regrows it
    while slot 1 runs.  third_slot: one more call on slot 2 (the context of three slots on one stream)."""
    s = [step("full", "C", 801, slot=1, wait=False), step("full_batch", "A", (802, 803, 804), slot=0, wait=False),
         step("fov_multi", "B", 805, slot=1, wait=False, offsets=OFFS3), step("full", "C", 806, slot=0, wait=False)]
    return s + ([step("full", "T", 807, slot=2, wait=False)] if third_slot else [])


def group_i():
    """Out of memory in the middle (UGSM_MEM_LIMIT_MB): a C pair, four C pairs refused right behind it, then A, four A, C."""
    return [step("full", "C", 901, wait=False), step("refused", "C", 902, what="nomem", n=4), step("full", "A", 903, wait=False),
            step("full_batch", "A", (904, 905, 906, 907), wait=False), step("full", "C", 908)]


GROUPS = {
    "a": (group_a, {0: ("grow_behind_unwaited", "shrink_warm", "nb_up", "nb_down", "no_wait")}),
    "b": (group_b, {0: ("nb_down", "nb_up", "checked_to_plain", "no_wait")}),
    "c": (group_c, {0: ("fovea_to_full", "full_to_fovea", "slot_to_host", "host_to_slot", "nb_up", "nb_down", "shrink_warm")}),
    "d": (group_d, {0: ("full_to_fovea", "fovea_to_full", "no_wait")}),
    "e": (group_e, {0: ("format_behind_unwaited", "lr_behind_unwaited", "shrink_warm", "no_wait")}),
    "f": (group_f, {0: ("format_behind_unwaited", "full_to_fovea", "fovea_to_full", "nb_up", "nb_down", "shrink_warm", "no_wait")}),
    "g": (group_g, {0: ("shrink_warm", "post_shrink", "post_grow", "no_wait")}),
    "h": (group_h, {0: ("grow_behind_unwaited", "nb_down", "no_wait"), 1: ("full_to_fovea", "shrink_warm", "no_wait")}),
    "i": (group_i, {0: ("shrink_warm", "nb_up", "nb_down", "grow_behind_unwaited", "no_wait")}),
}
WALK_SEEDS = (12, 13, 17)      # (seeds whose walks meet test_context_life_host.py's conditions: a seed that does not is replaced, never the condition)
# what every walk goes through: on slot 0 everything, on slot 1 everything but the blocking host-memory calls (they run on slot 0)
WALK_BOTH = ("grow_behind_unwaited", "shrink_warm", "nb_down", "nb_up", "checked_to_plain", "fovea_to_full", "full_to_fovea")
WALK_SLOT0 = WALK_BOTH + ("host_to_slot", "slot_to_host")
