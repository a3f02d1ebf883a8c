"""The cloud from the queue (ugsm_enqueue_*_cloud*, ugsm_done_cloud) on the device against the slot-level route on a second context:
ugsm_submit_full / ugsm_submit_foveated for the pair, then ugsm_point_cloud / ugsm_point_cloud_fovea_all -- byte for byte: the records, the
count, the level counts, and (device kind) the bytes past the records written untouched.  That route is pinned to tests/cloud_np.py and
tests/stack_cloud_np.py by test_gpu_cloud.py and test_gpu_stack_cloud.py.

Shapes: the smallest that exercise partial tiles and several pairs.  Full mode 160 x 120, 8 levels: the cloud tile is 32 x 64 sampled points,
so 5 strips x 2 chunks with a partial last chunk, and at sampling 3 (54 x 40) a partial strip and one partial chunk.  Foveated 320 x 240, 9
levels, 4 fovea levels: a 112 x 84 window, 3.5 strips x 2 chunks per level, every pair of a call at another offset, one clamped at the edge.

Compact clouds take min_conf = the median of the confidence plane of the call's FIRST pair (the pairs of a call share a spec) and a Z window
at the 5th and 95th percentile of its finite Z: the synthetic pairs' confidence never falls below 0.47, so a fixed threshold such as 0.3
would keep every point and test no compaction.  0 < count < dense is asserted for every pair."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cloud import P1, P2A, POISON

pytestmark = pytest.mark.gpu

EXTRA = 64          # records of poison behind every device cloud buffer
FULL = dict(W=160, H=120, levels=8, F=4)
FOVEA = dict(W=320, H=240, levels=9, F=4)
OFFSETS = [(0, 0), (23, -17), (-60, 40), (1000, 1000), (-31, 9), (8, 8), (-1000, 0)]     # (1000, 1000) and (-1000, 0): clamped at the image edge


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def geometry(fovea):
    return FOVEA if fovea else FULL


@pytest.fixture(scope="module")
def pairs():
    """Seven synthetic pairs per mode, seeds 1 .. 7."""
    from ug_stereomatcher_amd import synth
    out = {}
    for fovea in (False, True):
        g = geometry(fovea)
        out[fovea] = [synth.make_pair(g["W"], g["H"], synth.BASE_SEED + 1 + k)[:2] for k in range(7)]
    return out


class Ref:
    """The slot-level route on a context of its own: each pair's result (kept on the device), and its clouds on demand."""

    def __init__(self, lib, pairs, fovea, lr=0.0):
        g = geometry(fovea)
        self.lib, self.fovea, self.g = lib, fovea, g
        self.c = lib.Context(levels=g["levels"], fovea_levels=g["F"])
        if lr > 0:
            self.c.set_lr_check(lr)
        self.pairs = pairs
        self.res, self.marked, self.clouds = {}, {}, {}
        self.fw, self.fh = lib.fovea_dims(g["W"], g["H"], g["levels"], g["F"]) if fovea else (g["W"], g["H"])
        self.plane = (g["F"] if fovea else 1) * self.fw * self.fh

    def close(self):
        self.c.close()

    def result(self, k, off=(0, 0)):
        """(device image, device result, the result's three planes on the host) of pair k (foveated: at offset off)."""
        key = (k, tuple(off))
        if key not in self.res:
            c, g = self.c, self.g
            L, R = self.pairs[k]
            dL, dR = c.to_device(L), c.to_device(R)
            d_out = c.alloc(3 * self.plane * 4)
            if self.fovea:
                c.check(c.lib.ugsm_submit_foveated(c.handle, 0, dL, dR, g["W"], g["H"], 3 * g["W"], off[0], off[1], d_out, None, None))
            else:
                c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, g["W"], g["H"], 3 * g["W"], d_out))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            self.marked[key] = c.last_lr_marked(0)
            c.free(dR)
            self.res[key] = (dL, d_out, c.to_host(d_out, (3, self.plane), np.float32))
        return self.res[key]

    def dense(self, off, s):
        g = self.g
        if self.fovea:
            return self.lib.fovea_cloud_points(g["W"], g["H"], g["levels"], g["F"], off, s)
        return self.lib.cloud_points(g["W"], g["H"], s)

    def cloud(self, k, off, s, fmt, compact, min_conf=None, z=(None, None)):
        """(count, the records as bytes, level counts) of pair k's slot-level cloud."""
        key = (k, tuple(off), s, fmt, compact, min_conf, z)
        if key not in self.clouds:
            c, g, lib = self.c, self.g, self.lib
            dL, d_out, _ = self.result(k, off)
            params = lib.cloud_params(sampling=s, format=fmt, compact=compact, min_conf=min_conf, z_min=z[0], z_max=z[1])
            cap = self.dense(off, s)
            item = 32 if fmt == lib.UGSM_CLOUD_PCL32 else 16
            d_pts, d_cnt, d_lvl = c.alloc(cap * item), c.alloc(8), c.alloc(8 * g["F"])
            planes = [d_out + p * self.plane * 4 for p in range(3)]
            if self.fovea:
                n, per = c.point_cloud_fovea_all(*planes, g["W"], g["H"], off, dL, 3 * g["W"], P1, P2A, params, d_pts, cap, d_cnt, d_lvl)
            else:
                n, per = c.point_cloud(*planes, dL, g["W"], g["H"], 3 * g["W"], P1, P2A, params, d_pts, cap, d_cnt), []
            self.clouds[key] = (n, c.to_host(d_pts, (min(n, cap) * item,), np.uint8), per)
            for p in (d_pts, d_cnt, d_lvl):
                c.free(p)
        return self.clouds[key]

    def thresholds(self, k, off):
        """min_conf = the median of pair k's confidence plane, a Z window at the 5th and 95th percentile of its finite Z."""
        _, _, planes = self.result(k, off)
        n, rec, _ = self.cloud(k, off, 1, self.lib.UGSM_CLOUD_XYZRGB16, False)
        z = rec.view(np.float32).reshape(-1, 4)[:, 2]
        z = z[np.isfinite(z)]
        return float(np.median(planes[2])), (float(np.percentile(z, 5)), float(np.percentile(z, 95)))


@pytest.fixture(scope="module")
def refs(lib, pairs):
    made = {}

    def get(fovea, lr=0.0):
        if (fovea, lr) not in made:
            made[(fovea, lr)] = Ref(lib, pairs[fovea], fovea, lr)
        return made[(fovea, lr)]
    yield get
    for r in made.values():
        r.close()


def run_burst(lib, ref, kind, jobs, slots, batch, lr=0.0, formats=None):
    """jobs: one dict per pair -- k (the pair), off, the spec's fields (s, fmt, compact, min_conf, z), cap (device: cap_points; managed:
    max_points; None = the dense size), want_planes, plain (a plain managed pair, no cloud).  Enqueued back to back, flushed, drained.
    Returns one dict per pair: count, records (bytes), levels, stored, call_pairs, call_index, planes."""
    g, fovea = ref.g, ref.fovea
    W, H = g["W"], g["H"]
    out = []
    with lib.Context(levels=g["levels"], fovea_levels=g["F"], slots=slots, batch=batch) as c:
        if lr > 0:
            c.set_lr_check(lr)
        held = []
        for tag, j in enumerate(jobs):
            if formats:
                c.set_input_format(formats[tag])
            L, R = j.get("images") or ref.pairs[j["k"]]
            if j.get("plain"):
                (c.enqueue_foveated_managed(L, R, j["off"], False, tag) if fovea else c.enqueue_full_managed(L, R, tag))
                held.append(None)
                continue
            item = 32 if j["fmt"] == lib.UGSM_CLOUD_PCL32 else 16
            params = lib.cloud_params(sampling=j["s"], format=j["fmt"], compact=j["compact"], min_conf=j.get("min_conf"), z_min=j.get("z", (None, None))[0],
                                      z_max=j.get("z", (None, None))[1])
            cap = j.get("cap")
            if kind == "managed":
                spec = lib.queue_cloud(P1, P2A, params, max_points=cap or 0, want_planes=bool(j.get("want_planes")))
                (c.enqueue_foveated_cloud_managed(L, R, j["off"], spec, tag) if fovea else c.enqueue_full_cloud_managed(L, R, spec, tag))
                held.append(None)
            else:
                spec = lib.queue_cloud(P1, P2A, params)
                cap = ref.dense(j["off"], j["s"]) if cap is None else cap
                dL, dR = c.to_device(L), c.to_device(R)
                d_out = c.alloc(3 * ref.plane * 4)
                d_pts = c.to_device(np.full((cap + EXTRA) * item, POISON, np.uint8))
                d_cnt, d_lvl = c.to_device(np.full(1, -7, np.int64)), c.to_device(np.full(g["F"], -7, np.int64))
                if fovea:
                    c.enqueue_foveated_cloud(dL, dR, W, H, L.strides[0], j["off"], d_out, spec, d_pts, cap, d_cnt, tag, d_level_counts=d_lvl)
                else:
                    c.enqueue_full_cloud(dL, dR, W, H, L.strides[0], d_out, spec, d_pts, cap, d_cnt, tag)
                held.append((dL, dR, d_out, d_pts, d_cnt, d_lvl, cap, item))
        c.flush()
        for tag, j in enumerate(jobs):
            d = c.next_done(True)
            assert d is not None and d.tag == tag, (tag, d and d.tag)                       # enqueue order, tags intact
            r = dict(call_pairs=d.call_pairs, call_index=d.call_index, planes=None, count=None)
            if j.get("plain") or (kind == "managed" and j.get("want_planes")):
                assert d.result[0] and d.result[1] and d.result[2]
                r["planes"] = np.stack([p.copy() for p in c.managed_planes(d, [(ref.plane,)] * 3)])
            elif kind == "managed":
                assert not d.result[0] and not d.result[1] and not d.result[2]               # not downloaded
            if j.get("plain"):
                with pytest.raises(lib.UgsmError) as e:
                    c.done_cloud()
                assert e.value.status == lib.UGSM_ERR_STATE
            elif kind == "managed":
                rec, n, per = c.done_cloud()
                r.update(count=n, stored=rec.size, records=rec.view(np.uint8).copy(), levels=per)
            else:
                dL, dR, d_out, d_pts, d_cnt, d_lvl, cap, item = held[tag]
                n = int(c.to_host(d_cnt, (1,), np.int64)[0])
                raw = c.to_host(d_pts, ((cap + EXTRA) * item,), np.uint8)
                stored = min(n, cap)
                assert (raw[stored * item:] == POISON).all(), f"pair {tag}: a byte past the records written was touched"
                r.update(count=n, stored=stored, records=raw[:stored * item], levels=c.to_host(d_lvl, (g["F"],), np.int64).tolist() if fovea else [],
                         planes=c.to_host(d_out, (3, ref.plane), np.float32))
            out.append(r)
        assert c.next_done(True) is None
    return out


def check_against_ref(ref, jobs, got, lib):
    for tag, (j, r) in enumerate(zip(jobs, got)):
        if j.get("plain"):
            continue
        n, rec, per = ref.cloud(j["k"], j["off"], j["s"], j["fmt"], j["compact"], j.get("min_conf"), j.get("z", (None, None)))
        item = 32 if j["fmt"] == lib.UGSM_CLOUD_PCL32 else 16
        what = f"pair {tag} (seed {j['k']}, off {j['off']})"
        print(f"{what}: count {r['count']} (slot-level {n}), stored {r['stored']}, call of {r['call_pairs']}")
        assert r["count"] == n, what
        assert r["levels"] == per, what
        stored = min(n, j["cap"]) if j.get("cap") is not None else n
        assert r["stored"] == stored, what
        assert np.array_equal(r["records"], rec[:stored * item]), what
        if r["planes"] is not None:
            assert np.array_equal(r["planes"].view(np.uint32), ref.result(j["k"], j["off"])[2].view(np.uint32)), what   # the pair's result itself


def burst_jobs(ref, lib, variant, n=7, groups=(3, 4)):
    """n pairs with different seeds (and offsets); compact variants: one threshold per intended call, from its first pair."""
    s, fmt, compact = {"dense_pcl32": (1, lib.UGSM_CLOUD_PCL32, False), "compact_xyzrgb16": (1, lib.UGSM_CLOUD_XYZRGB16, True),
                       "compact_s3": (3, lib.UGSM_CLOUD_PCL32, True)}[variant]
    jobs, first = [], 0
    bounds = np.cumsum(groups).tolist()
    for t in range(n):
        if t in bounds:
            first = t
        j = dict(k=t % 7, off=OFFSETS[t % 7] if ref.fovea else (0, 0), s=s, fmt=fmt, compact=compact)
        if compact:
            j["min_conf"], j["z"] = ref.thresholds(first % 7, OFFSETS[first % 7] if ref.fovea else (0, 0))
        jobs.append(j)
    return jobs


def assert_compacts(ref, jobs, got):
    for j, r in zip(jobs, got):
        if j.get("compact"):
            assert 0 < r["count"] < ref.dense(j["off"], j["s"]), (r["count"], ref.dense(j["off"], j["s"]))


@pytest.mark.parametrize("variant", ["dense_pcl32", "compact_xyzrgb16", "compact_s3"])
@pytest.mark.parametrize("kind", ["device", "managed"])
@pytest.mark.parametrize("fovea", [False, True], ids=["full", "foveated"])
def test_a_burst_of_seven_pairs_gives_each_pair_its_slot_level_cloud(lib, refs, fovea, kind, variant):
    """slots 2, batch 4: seven pairs enqueued back to back and flushed go out in more than one call, one of at least three pairs."""
    ref = refs(fovea)
    jobs = burst_jobs(ref, lib, variant)
    got = run_burst(lib, ref, kind, jobs, slots=2, batch=4)
    calls = {r["call_index"]: r["call_pairs"] for r in got}
    assert len(calls) > 1 and max(calls.values()) >= 3 and sum(calls.values()) == 7, calls
    check_against_ref(ref, jobs, got, lib)
    assert_compacts(ref, jobs, got)


@pytest.mark.parametrize("kind", ["device", "managed"])
@pytest.mark.parametrize("fovea", [False, True], ids=["full", "foveated"])
def test_a_cap_keeps_the_first_records_and_the_full_count(lib, refs, fovea, kind):
    """cap_points (device) / max_points (managed) at about 40 % of the call's smallest count: the first cap records are the slot-level
    cloud's, count is the full size, stored == cap, nothing is written past the cap (device: the poison behind it)."""
    ref = refs(fovea)
    jobs = burst_jobs(ref, lib, "compact_xyzrgb16", n=4, groups=(4,))
    counts = [ref.cloud(j["k"], j["off"], j["s"], j["fmt"], True, j["min_conf"], j["z"])[0] for j in jobs]
    cap = int(0.4 * min(counts))
    assert cap > 0
    for j in jobs:
        j["cap"] = cap
    got = run_burst(lib, ref, kind, jobs, slots=1, batch=4)
    check_against_ref(ref, jobs, got, lib)
    for r, n in zip(got, counts):
        assert r["count"] == n > cap and r["stored"] == cap


@pytest.mark.parametrize("fovea", [False, True], ids=["full", "foveated"])
def test_managed_clouds_with_and_without_planes_between_plain_pairs(lib, refs, fovea):
    """want_planes 0 then 1, interleaved with plain managed pairs in one burst: with 1 the planes equal the plain pair's, with 0 result[] is
    NULL (checked in run_burst); order and tags are intact."""
    ref = refs(fovea)
    base = burst_jobs(ref, lib, "compact_xyzrgb16", n=1, groups=(1,))[0]
    jobs = []
    for want, plain, k in [(0, False, 0), (0, True, 1), (1, False, 1), (1, False, 2), (0, True, 2), (0, False, 0), (1, False, 0)]:
        jobs.append(dict(base, k=k, off=OFFSETS[k] if fovea else (0, 0), want_planes=want, plain=plain))
    got = run_burst(lib, ref, "managed", jobs, slots=2, batch=4)
    check_against_ref(ref, jobs, got, lib)
    plain = {j["k"]: r["planes"] for j, r in zip(jobs, got) if j["plain"]}
    seen = 0
    for j, r in zip(jobs, got):
        if not j["plain"] and j["want_planes"] and j["k"] in plain:
            assert np.array_equal(r["planes"].view(np.uint32), plain[j["k"]].view(np.uint32))
            seen += 1
    assert seen == 2
    assert len({r["call_index"] for r in got}) >= 5                                      # plain pairs and the other want_planes end the groups


@pytest.mark.parametrize("kind", ["device", "managed"])
def test_a_bgr8_pair_and_its_rgb8_twin_give_the_same_cloud(lib, refs, kind):
    """The colour words follow the input format captured at enqueue: the same scene as bgr8 (channels swapped on the host) and as rgb8, in one
    burst -- two calls, one cloud."""
    ref = refs(False)
    base = burst_jobs(ref, lib, "compact_xyzrgb16", n=1, groups=(1,))[0]
    L, R = ref.pairs[0]
    swapped = (np.ascontiguousarray(L[:, :, ::-1]), np.ascontiguousarray(R[:, :, ::-1]))
    jobs = [dict(base, images=swapped), dict(base)]
    got = run_burst(lib, ref, kind, jobs, slots=2, batch=4, formats=[lib.UGSM_INPUT_BGR8, lib.UGSM_INPUT_RGB8])
    assert got[0]["call_index"] != got[1]["call_index"]
    check_against_ref(ref, jobs, got, lib)
    assert np.array_equal(got[0]["records"], got[1]["records"]) and got[0]["count"] == got[1]["count"] > 0


def pixel_masks(ref, k, off, rec_dense):
    """Per pixel of pair k's result: in the dense cloud at all (not covered by a finer level), and its record finite -- from the dense
    slot-level cloud, whose order is level by level, column outer, row inner, the covered pixels left out."""
    import stack_cloud_np as sn
    g = ref.g
    F = g["F"] if ref.fovea else 1
    xyz = rec_dense.view(np.float32).reshape(-1, 4)[:, :3]
    fin = np.isfinite(xyz).all(axis=1)
    inc = np.zeros((F, ref.fh, ref.fw), bool)
    finite = np.zeros((F, ref.fh, ref.fw), bool)
    at = 0
    for lv in range(F):
        if ref.fovea:
            cols, rows = sn.covered(g["W"], g["H"], F, lv, off)
            unc = ~np.outer(cols, rows)                                                  # (fw, fh): column outer, row inner
        else:
            unc = np.ones((ref.fw, ref.fh), bool)
        n = int(unc.sum())
        f = np.zeros((ref.fw, ref.fh), bool)
        f[unc] = fin[at:at + n]
        at += n
        inc[lv], finite[lv] = unc.T, f.T
    assert at == fin.size
    return inc.reshape(-1), finite.reshape(-1)


@pytest.mark.parametrize("kind", ["device", "managed"])
@pytest.mark.parametrize("fovea", [False, True], ids=["full", "foveated"])
def test_with_the_lr_check_on_a_compact_cloud_leaves_the_marked_pixels_out(lib, refs, fovea, kind):
    """ugsm_set_lr_check before the first enqueue: a compact cloud with min_conf > 0 has exactly dense - marked - otherwise-dropped points and
    equals the slot-level cloud of the checked result."""
    tau = 0.5
    ref, plain = refs(fovea, tau), refs(fovea)
    offs = OFFSETS if fovea else [(0, 0)] * 7
    min_conf = float(np.median(plain.result(0, offs[0])[2][2]))
    assert min_conf > 0
    xyz16 = lib.UGSM_CLOUD_XYZRGB16
    jobs = [dict(k=k, off=offs[k], s=1, fmt=xyz16, compact=True, min_conf=min_conf) for k in range(3)]
    got = run_burst(lib, ref, kind, jobs, slots=2, batch=4, lr=tau)
    check_against_ref(ref, jobs, got, lib)
    for j, r in zip(jobs, got):
        conf_c, conf_u = ref.result(j["k"], j["off"])[2][2], plain.result(j["k"], j["off"])[2][2]
        inc, finite = pixel_masks(ref, j["k"], j["off"], ref.cloud(j["k"], j["off"], 1, xyz16, False)[1])
        marked = inc & (conf_c != conf_u)                                                # the check zeroed the pixel's confidence
        assert marked.any() and (conf_c[marked] == 0).all()
        if not fovea:
            assert int(marked.sum()) == ref.marked[(j["k"], (0, 0))]
        otherwise = inc & ~marked & ~(finite & (conf_c >= min_conf))
        dense = ref.dense(j["off"], 1)
        print(f"seed {j['k']}: dense {dense}, marked {int(marked.sum())}, otherwise dropped {int(otherwise.sum())}, count {r['count']}")
        assert int(inc.sum()) == dense
        assert r["count"] == dense - int(marked.sum()) - int(otherwise.sum())
        assert 0 < r["count"] < dense


def test_every_call_one_pair(lib, refs):
    """slots 1, batch 1: the single-pair route of the matcher, the cloud behind each pair's match.  (Two pairs: (slots + 1) x batch is what
    such a context lets a host have outstanding.)"""
    for fovea in (False, True):
        ref = refs(fovea)
        jobs = burst_jobs(ref, lib, "compact_xyzrgb16", n=2, groups=(2,))
        for kind in ("device", "managed"):
            got = run_burst(lib, ref, kind, jobs, slots=1, batch=1)
            assert [r["call_pairs"] for r in got] == [1, 1]
            check_against_ref(ref, jobs, got, lib)


@pytest.mark.parametrize("kind", ["device", "managed"])
def test_sixteen_pairs_in_one_call(lib, refs, kind):
    """batch 16 and 16 pairs: the full table, each row with its own window offset."""
    ref = refs(True)
    jobs = burst_jobs(ref, lib, "compact_xyzrgb16", n=16, groups=(16,))
    got = run_burst(lib, ref, kind, jobs, slots=1, batch=16)
    assert [r["call_pairs"] for r in got] == [16] * 16
    check_against_ref(ref, jobs, got, lib)
    assert_compacts(ref, jobs, got)
