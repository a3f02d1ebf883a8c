"""The conditions on the inputs of tests/test_gpu_context_life.py, checked on the CPU, so that a green GPU run means something: every script
contains the transitions it is there for (computed from its steps), any two expected arrays of a script differ in more than half of their
elements (a stale or misrouted result cannot pass for another's), every filter of every step both keeps and drops, and the expected values
that tests/context_life.py hands out are what the per-feature restatements give when they are called directly."""
from collections import Counter

import numpy as np
import pytest

import cloud_np as cn
import coarse_np as cs
import context_life as cl
import depth_np as dn
import encode_np as en
import fovea_seeded_np as fs
import reconstruct_multi_np as rm
import seeded_np as sn
import warp_np as wn
from conftest import assert_bit_equal
from test_gpu_cloud import P1, P2A

SCRIPTS = {**{name: make() for name, (make, _) in cl.GROUPS.items()}, "h3": cl.group_h(True), **{f"walk{seed}": cl.walk(seed) for seed in cl.WALK_SEEDS}}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def exp(orc):
    return cl.Expect(orc)


def test_every_frame_has_a_pyramid_and_a_fovea(lib):
    for name, (W, H) in cl.FRAMES.items():
        w, h = lib.level_dims(W, H, cl.LEVELS)                             # (raises for a size the context's levels refuse)
        fw, fh = lib.fovea_dims(W, H, cl.LEVELS, cl.FOVEA)
        assert min(w) >= 1 and min(h) >= 1 and fw * fh * 2 <= W * H, name
    with pytest.raises(lib.UgsmError):
        lib.level_dims(11, 9, cl.LEVELS)                                   # the refused step's frame has none


@pytest.mark.parametrize("name", SCRIPTS)
def test_scripts_are_well_formed(name):
    script = SCRIPTS[name]
    pairs = [p for s in script for p in s.pairs]
    assert len(pairs) == len(set(pairs)), "every step brings image pairs of its own"
    for i, s in enumerate(script):
        fam, _, blocking = cl.KINDS[s.kind]
        assert not blocking or (s.slot == 0 and s.wait_after), (i, str(s))
        needs = {"full_seeded": ("full", "fine"), "fine": ("coarse",), "fov_warm": ("fov_batch", "fov_multi"), "fovea_fine": ("fovea_coarse",),
                 "cloud": ("full",), "depth16u": ("full",), "warp_right": ("full",), "residual": ("full",)}.get(s.kind)
        if s.kind == "fovea_coarse" and not s.arg("refused"):
            needs = ("pyramids",)
        if needs is None:
            assert s.src < 0, (i, str(s))
            continue
        src = script[s.src]
        assert 0 <= s.src < i and src.kind in needs and src.slot == s.slot and src.frame == s.frame, (i, str(s), str(src))
        if s.kind in ("fovea_coarse", "fovea_fine"):                       # the pyramids are still the slot's
            between = [t for t in script[s.src + 1:i] if t.slot == s.slot and cl.KINDS[t.kind][0] not in ("setting", "refused", "phase")]
            assert not between, (i, [str(t) for t in between])
        assert cl.settings(script)[s.src] == cl.settings(script)[i], "a step and what it hangs on run under the same settings"
    assert cl.settings(script + [cl.step("full", "A", 0)])[-1][:2] == (cl.RGB8, 0.0), "the settings are put back at the end: rgb8, check off"


@pytest.mark.parametrize("name", cl.GROUPS)
def test_scripted_groups_contain_their_transitions(name):
    make, wanted = cl.GROUPS[name]
    found = cl.transitions(make())
    for slot, names in wanted.items():
        for t in names:
            assert found.get(slot, {}).get(t, 0) >= 1, f"group {name}, slot {slot}: no {t} in {found}"
    if name == "e":
        assert found[0]["format_behind_unwaited"] >= 4                     # bgr8, mono8, rgb32f, and back to rgb8


@pytest.mark.parametrize("seed", cl.WALK_SEEDS)
def test_walks_contain_every_kind_and_transition(seed):
    script = cl.walk(seed)
    assert script == cl.walk(seed), "a walk is a plain function of its seed"
    kinds = Counter(s.kind for s in script)
    assert all(kinds[k] >= 2 for k in cl.KINDS), {k: kinds[k] for k in cl.KINDS if kinds[k] < 2}
    assert {s.frame for s in script if cl.KINDS[s.kind][0] != "setting"} == set(cl.WALK_FRAMES)
    found = cl.transitions(script)
    for slot, names in ((0, cl.WALK_SLOT0), (1, cl.WALK_BOTH)):
        for t in names:
            assert found[slot].get(t, 0) >= 1, f"walk {seed}, slot {slot}: no {t}"
        assert found[slot]["no_wait"] >= 10, f"walk {seed}, slot {slot}: {found[slot]['no_wait']} hand-overs without a wait"
    assert sum(f.get("format_behind_unwaited", 0) for f in found.values()) >= 1 and sum(f.get("lr_behind_unwaited", 0) for f in found.values()) >= 1
    waited = [s.wait_after for s in script if cl.KINDS[s.kind][0] != "setting" and not cl.KINDS[s.kind][2]]
    assert 0.15 < np.mean(waited) < 0.5, np.mean(waited)                   # (drawn with probability 1/3)


def _arrays(exp, script):
    """(step, name, array) of every expected float array of the script."""
    out = []
    for i in range(len(script)):
        for name, v in exp.expected(script, i).items():
            if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.size > 16:
                out.append((i, name, v))
    return out


@pytest.mark.parametrize("name", SCRIPTS)
def test_expected_values_are_distinct(exp, name):
    """Any two expected arrays of one shape differ in more than half of their elements.  Not compared: a warm call's stack with the prior stack
    it starts from (its upper row blocks ARE the prior's), and the row block F-1 of the stacks of one pair's windows (the same whole-frame level)."""
    script = SCRIPTS[name]
    by_shape = {}
    for i, nm, v in _arrays(exp, script):
        by_shape.setdefault(v.shape, []).append((i, nm, v))
    compared = 0
    for shape, group in by_shape.items():
        for a in range(len(group)):
            for b in range(a + 1, len(group)):
                (i, ni, x), (j, nj, y) = group[a], group[b]
                if script[j].kind == "fov_warm" and script[j].src == i:
                    continue
                if i == j and ni.startswith("stack") and nj.startswith("stack"):
                    x, y = x[:, :cl.FOVEA - 1], y[:, :cl.FOVEA - 1]
                differ = np.mean(x.view(np.uint32) != y.view(np.uint32))
                assert differ > 0.5, f"{name}: step {i} {ni} and step {j} {nj} differ in {differ:.2f} of their elements"
                compared += 1
    assert compared > 0


@pytest.mark.parametrize("name", SCRIPTS)
def test_every_filter_keeps_and_drops(exp, name):
    script = SCRIPTS[name]
    for i, s in enumerate(script):
        W, H = s.size
        e = exp.expected(script, i)
        if s.kind == "cloud":
            assert 0 < e["cloud"].size < cn.cloud_points(W, H, 1), (i, e["cloud"].size)
        if s.kind == "depth16u":
            dn.assert_both_branches(e["depth"] != 0, f"{name} step {i}")
            assert e["valid"] == int((e["depth"] != 0).sum())
        if s.kind == "full_checked":
            for b in range(s.n):
                assert all(0 < m < W * H for m in e[f"marked{b}"]), (i, e[f"marked{b}"])
        if s.kind in ("full", "full_host") and cl.lr_on(cl.settings(script)[i]):
            F = exp.full(s.frame, s.pairs[0], cl.settings(script)[i][0])
            zeroed = int(((e["out"][2] == 0) & (F[2] != 0)).sum())
            assert 0 < zeroed < W * H, (i, zeroed)
        if s.kind == "fov_multi_checked":
            fw, fh = exp.orc.fovea_geometry(W, H, cl.LEVELS, cl.FOVEA)[:2]
            for j in range(len(s.arg("offsets"))):
                assert 0 < sum(e[f"marked{j}"]) < cl.FOVEA * fw * fh and max(e[f"marked{j}"]) > 0, (i, e[f"marked{j}"])


# ---- a pin on the expected values: one cheap step per kind against the restatement called directly ---------------------------------------

PIN = [
    cl.step("full", "A", 9001), cl.step("full_batch", "A", (9002, 9003)), cl.step("full_host", "A", 9004), cl.step("full_batch_host", "A", (9005, 9006)),
    cl.step("full_checked", "A", (9007,), tau=cl.TAU), cl.step("full_seeded", "A", 9008, src=0, s=2), cl.step("coarse", "A", 9009, e=3),
    cl.step("fine", "A", src=6, e=3), cl.step("fov_batch", "A", (9010,), offsets=((12, -7),), pyr=True), cl.step("fov_host", "A", 9011, offsets=((-9, 4),), pyr=False),
    cl.step("fov_multi", "A", 9012, offsets=((0, 0), (25, 10))), cl.step("fov_multi_checked", "A", 9013, offsets=((5, 5),), tau=cl.TAU),
    cl.step("fov_warm", "A", 9014, src=8, offsets=((3, 3),), s=1), cl.step("pyramids", "A", 9015), cl.step("fovea_coarse", "A", src=13),
    cl.step("fovea_fine", "A", src=14, off=(7, -3)), cl.step("cloud", "A", src=0), cl.step("depth16u", "A", src=0), cl.step("warp_right", "A", src=0),
    cl.step("residual", "A", src=0), cl.step("stage_iterate", "A", 9016), cl.step("stage_smooth", "A", 9017), cl.step("stage_pyramid", "A", 9018, level=2),
    cl.step("set_format", fmt=cl.MONO8), cl.step("full", "A", 9019), cl.step("set_format", fmt=cl.RGB8), cl.step("set_lr", tau=cl.TAU, modes=1),
    cl.step("full", "A", 9020), cl.step("set_lr", tau=0.0, modes=0), cl.step("refused", "A", 9021, what="stride"),
]


def _pair(p, frame="A"):
    from ug_stereomatcher_amd import synth
    return synth.make_pair(*cl.FRAMES[frame], synth.BASE_SEED + cl.SEED + p)[:2]


def test_expected_values_are_the_restatements_called_directly(exp, orc):
    assert {s.kind for s in PIN} == set(cl.KINDS)
    W, H = cl.FRAMES["A"]
    lv, F = cl.LEVELS, cl.FOVEA
    e = [exp.expected(PIN, i) for i in range(len(PIN))]
    full0 = orc.match_full(*_pair(9001), lv)
    assert_bit_equal(e[0]["out"], full0, "full")
    assert_bit_equal(e[1]["out1"], orc.match_full(*_pair(9003), lv), "full_batch, pair 1")
    assert_bit_equal(e[2]["out"], orc.match_full(*_pair(9004), lv), "full_host")
    assert_bit_equal(e[3]["out0"], orc.match_full(*_pair(9005), lv), "full_batch_host, pair 0")
    L, R = _pair(9007)
    fwd, bwd = orc.match_full(L, R, lv), orc.match_full(R, L, lv)
    (cf, nf), (cb, nb) = orc.lr_check(fwd, bwd, cl.TAU), orc.lr_check(bwd, fwd, cl.TAU)
    assert_bit_equal(e[4]["out0"], cf, "full_checked, forward")
    assert_bit_equal(e[4]["back0"], cb, "full_checked, backward")
    assert e[4]["marked0"] == (nf, nb)
    assert_bit_equal(e[4]["out0"][:2], fwd[:2], "the check leaves dx, dy alone")
    assert_bit_equal(e[5]["out"], sn.seeded_oracle(orc, *_pair(9008), full0, 2, lv), "full_seeded")
    state = cs.coarse_oracle(orc, *_pair(9009), 3, lv)
    w, h = orc.level_dims(W, H, lv)
    assert_bit_equal(e[6]["state"], state, "coarse")
    assert_bit_equal(e[6]["full"], cs.prolong_np(state, (list(w[:4]), list(h[:4]))), "coarse, the prolongation")
    assert_bit_equal(e[7]["out"], cs.fine_oracle(orc, *_pair(9009), state, 3, lv), "fine")
    assert_bit_equal(e[7]["out"], orc.match_full(*_pair(9009), lv), "the two halves give the whole call")
    stack, pl, pr = orc.match_foveated(*_pair(9010), lv, F, 12, -7, want_pyr=True)
    for name, want in (("stack0", stack), ("pyrL0", pl), ("pyrR0", pr)):
        assert_bit_equal(e[8][name], want, f"fov_batch {name}")
    assert_bit_equal(e[9]["stack0"], orc.match_foveated(*_pair(9011), lv, F, -9, 4)[0], "fov_host")
    assert set(e[9]) == {"stack0"}
    stacks = [orc.match_foveated(*_pair(9012), lv, F, ox, oy)[0] for ox, oy in ((0, 0), (25, 10))]
    assert_bit_equal(e[10]["stack1"], stacks[1], "fov_multi, window 1")
    assert_bit_equal(e[10]["full"], rm.reconstruct_multi(orc, stacks, W, H, lv, ((0, 0), (25, 10))), "fov_multi, the reconstruction")
    L, R = _pair(9013)
    S, B = orc.match_foveated(L, R, lv, F, 5, 5)[0], orc.match_foveated(R, L, lv, F, 5, 5)[0]
    for k in range(F):
        lvl, m = orc.lr_check(np.ascontiguousarray(S[:, k]), np.ascontiguousarray(B[:, k]), cl.TAU)
        assert_bit_equal(e[11]["stack0"][:, k], np.stack([S[0, k], S[1, k], lvl[2]]), f"fov_multi_checked, level {k}")
        assert e[11]["marked0"][k] == m
    assert_bit_equal(e[12]["stack0"], fs.warm_oracle(orc, *_pair(9014), stack, lv, (12, -7), (3, 3), 1), "fov_warm")
    assert e[13] == {}
    assert_bit_equal(e[14]["state"], cs.coarse_oracle(orc, *_pair(9015), F - 1, lv), "fovea_coarse")
    assert_bit_equal(e[15]["stack0"], orc.match_foveated(*_pair(9015), lv, F, 7, -3)[0], "fovea_fine")
    L, R = _pair(9001)
    z = orc.triangulate(full0[0], full0[1], P1, P2A)[2]
    zf, cf_ = z[np.isfinite(z)], full0[2][np.isfinite(full0[2])]
    kw = dict(min_conf=float(np.percentile(cf_, 30)), z_min=float(np.percentile(zf, 10)), z_max=float(np.percentile(zf, 90)))
    assert e[16]["cloud"].tobytes() == cn.cloud(orc, full0[0], full0[1], L, P1, P2A, conf=full0[2], compact=True, **kw).tobytes(), "cloud"
    kw = dict(fmt=dn.FMT_16U, unit=60.0 / float(np.percentile(z[np.isfinite(z) & (z > 0)], 80)), min_conf=float(np.percentile(cf_, 10)))
    img, valid = dn.depth_image(orc, full0[0], full0[1], P1, P2A, conf=full0[2], **kw)
    dn.assert_image_equal(e[17]["depth"], img, "depth16u")
    assert e[17]["valid"] == int(valid.sum())
    Rw = wn.warp(wn.planes(R), full0[0], full0[1])
    assert_bit_equal(e[18]["warp"], Rw, "warp_right")
    assert e[19]["sums"].tobytes() == wn.residual_sums(wn.planes(L), Rw, full0[2]).tobytes(), "residual"
    wd = orc.weighted_difference(np.stack([wn.planes(L)[0], wn.planes(L)[1], full0[2]]), np.stack([Rw[0], Rw[1], full0[2]]))
    assert_bit_equal(e[19]["quotient"][:2], np.array(wd[:2], np.float32), "residual, S / C against weighted_difference")
    L, R = _pair(9016)
    d = exp.stage_field(PIN[20])
    assert_bit_equal(e[20]["field"], orc.iterate_level(orc.rgb_to_planes(L), orc.rgb_to_planes(R), d, 4, 5, False, 1, 2)[0], "stage_iterate")
    d = exp.stage_field(PIN[21])
    for _ in range(5):
        d = orc.smooth_pass(d)
    assert_bit_equal(e[21]["field"], orc.box3(d), "stage_smooth")
    assert_bit_equal(e[22]["level"], orc.pyramid(orc.rgb_to_planes(_pair(9018)[0]), lv)[2], "stage_pyramid")
    L, R = _pair(9019)
    mono = [en.to_rgb8(en.encode(a, en.MONO8), en.MONO8) for a in (L, R)]
    assert_bit_equal(e[24]["out"], orc.match_full(*mono, lv), "full in mono8: the rgb8 call on the conversion")
    assert np.mean(e[24]["out"].view(np.uint32) != orc.match_full(L, R, lv).view(np.uint32)) > 0.5, "mono8 is not rgb8"
    L, R = _pair(9020)
    fwd, bwd = orc.match_full(L, R, lv), orc.match_full(R, L, lv)
    assert_bit_equal(e[27]["out"], orc.lr_check(fwd, bwd, cl.TAU)[0], "full under the context's LR check")
    assert e[29] == {"status": cl.SIZE_MISMATCH}
