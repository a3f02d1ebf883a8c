"""Accepted configurations on the device, against the CPU oracle bit for bit (product library, libugsm.so).

tests/test_config_space_host.py proves on the host that every level of every accepted configuration has a shipped K-cost kernel in its
plan.  Here the same configurations run: the cells that used to skip their cost step (march_min_pixels above k_cost_march4's reach, batched
calls whose launches outgrow it, UGSM_SMALL_MASK=0), a seeded random sweep of public configurations with the plan of every level checked
before the call, and the call pattern of the `alone` dimension that had no test: a second call on the slot whose stream a lone call has
borrowed."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_config_space_host import BATCH, MARCH_MIN, SMALL_MAX, plan_problems

pytestmark = pytest.mark.gpu

COST_NAMES = {1: "k_cost_march", 2: "k_cost_small", 4: "k_cost_march4"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture
def orc16(orc):
    orc.set_num_threads(16)
    yield orc
    orc.set_num_threads(8)


def _pairs(W, H, n, seed0):
    from ug_stereomatcher_amd import synth
    return [synth.make_pair(W, H, synth.BASE_SEED + seed0 + 11 * j)[:2] for j in range(n)]


def _full(c, pairs, W, H, slot=0):
    """The pairs as one ugsm_submit_full_batch call (one pair: ugsm_submit_full) on `slot`."""
    dL = [c.to_device(L) for L, _ in pairs]
    dR = [c.to_device(R) for _, R in pairs]
    dO = [c.alloc(3 * W * H * 4) for _ in pairs]
    try:
        if len(pairs) == 1:
            c.check(c.lib.ugsm_submit_full(c.handle, slot, dL[0], dR[0], W, H, 3 * W, dO[0]))
        else:
            c.submit_full_batch(slot, dL, dR, W, H, 3 * W, dO)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(p, (3, H, W)) for p in dO]
    finally:
        for p in dL + dR + dO:
            c.free(p)


def _foveated(c, lib, pairs, W, H, lv, F, offs, slot=0):
    fw, fh = lib.fovea_dims(W, H, lv, F)
    dL = [c.to_device(L) for L, _ in pairs]
    dR = [c.to_device(R) for _, R in pairs]
    dS = [c.alloc(3 * F * fh * fw * 4) for _ in pairs]
    try:
        c.submit_foveated_batch(slot, dL, dR, W, H, 3 * W, offs, dS)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(p, (3, F, fh, fw)) for p in dS]
    finally:
        for p in dL + dR + dS:
            c.free(p)


def _cost_launches(c):
    """{level: {K-cost kernel: launches}} of slot 0's harvested calls (profile_events = 2)."""
    out = {}
    for s in c.kernel_stats():
        if s["name"].startswith("k_cost") and s["launches"] > 0:
            out.setdefault(s["level"], {})[s["name"]] = s["launches"]
    return out


def _assert_every_level_ran_its_planned_cost_kernel(lib, c, W, H, lv, what, alone, **cfg):
    """Every level's K-cost ran as the plan says, once per iteration (one pair per call)."""
    got = _cost_launches(c)
    w, h = lib.level_dims(W, H, lv)
    for i in range(lv):
        want = COST_NAMES.get(lib.plan_level(w[i], h[i], alone=alone, **cfg)["cost_kernel"])
        assert got.get(i) == {want: lib.level_iterations(i)}, f"{what}: level {i} ({w[i]}x{h[i]}) ran {got.get(i)}, planned {want}"


def _assert_plans_complete(lib, sizes, what, **cfg):
    for (w, h) in sizes:
        for alone in (True, False):
            p = lib.plan_level(w, h, alone=alone, **cfg)
            bad = plan_problems(p, w, h, cfg.get("batch", 0))
            assert not bad, f"{what}: the plan of {w}x{h} (alone={alone}): {bad}"


# ---- the cells that had no K-cost in libugsm.so ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair_3000(orc):
    from ug_stereomatcher_amd import synth
    L, R, _, _ = synth.make_pair(3000, 2000, synth.BASE_SEED + 9101)
    orc.set_num_threads(16)
    try:
        return L, R, orc.match_full(L, R, 14), orc.match_foveated(L, R, 14, 7, 140, -90)[0]
    finally:
        orc.set_num_threads(8)


def test_march_min_above_march4_reach_full_3000x2000(lib, pair_3000):
    """march_min_pixels = 10^7 on a 3000 x 2000 pair: level 0 (6.0 Mpx), beyond k_cost_march4's 3 Mpx and below the threshold, marches.
    The launch statistics show every level's K-cost, once per iteration, as planned."""
    L, R, exp, _ = pair_3000
    W, H, lv = 3000, 2000, 14
    cfg = dict(march_min_pixels=10_000_000)
    _assert_plans_complete(lib, zip(*lib.level_dims(W, H, lv)), f"{cfg}", **cfg)
    assert lib.plan_level(W, H, **cfg)["cost_kernel"] == 1
    with lib.Context(levels=lv, profile_events=2, **cfg) as c:
        got = _full(c, [(L, R)], W, H)[0]
        _assert_every_level_ran_its_planned_cost_kernel(lib, c, W, H, lv, f"3000x2000 full, {cfg}", True, **cfg)
    assert_bit_equal(got, exp, f"3000x2000 full, {cfg}")


def test_march_min_above_march4_reach_foveated_3000x2000(lib, pair_3000):
    """The same configuration in foveated mode.  Its fine levels work on the 373 x 248 window and its coarse levels are those of the full
    frame from level F-1 = 6 down, all within the reach of k_cost_march4 and the latency kernels: the configuration must serve this
    mode as it did before."""
    L, R, _, exp = pair_3000
    W, H, lv, F = 3000, 2000, 14, 7
    cfg = dict(march_min_pixels=10_000_000)
    with lib.Context(levels=lv, fovea_levels=F, **cfg) as c:
        got = _foveated(c, lib, [(L, R)], W, H, lv, F, [(140, -90)])[0]
    assert_bit_equal(got, exp, f"3000x2000 foveated at (140, -90), {cfg}")


@pytest.mark.parametrize("W,H,n", [(1920, 1080, 2), (640, 480, 16)])
def test_batched_launches_beyond_march4_reach(lib, orc16, W, H, n):
    """march_min_pixels = 2^31 - 1 with a batch call whose launches hold more than 3 Mpx (2 x 1080p: 4.1 Mpx; 16 x 640 x 480: 4.9 Mpx),
    every pair a different image, every pair against the oracle."""
    lv = 14
    cfg = dict(march_min_pixels=2**31 - 1, batch=n)
    _assert_plans_complete(lib, zip(*lib.level_dims(W, H, lv)), f"{cfg}", **cfg)
    assert lib.plan_level(W, H, **cfg)["cost_kernel"] == 1
    pairs = _pairs(W, H, n, 9200 + W)
    with lib.Context(levels=lv, slots=2, **cfg) as c:
        got = _full(c, pairs, W, H, slot=1)
    for b, (L, R) in enumerate(pairs):
        assert_bit_equal(got[b], orc16.match_full(L, R, lv), f"{W}x{H} batch of {n}, {cfg}, pair {b}")


@pytest.mark.parametrize("alone", ["1", "0"])
@pytest.mark.parametrize("W,H,lv", [(640, 480, 14), (160, 120, 8)])
def test_small_mask_zero_down_to_the_smallest_levels(lib, orc, monkeypatch, W, H, lv, alone):
    """UGSM_SMALL_MASK=0 (development: no latency kernels) on the product library: the levels k_cost_small would have taken march, down
    to the 5 x 4 and 8 x 6 levels; once as a call alone on the chip, once as one that shares it (UGSM_ALONE)."""
    monkeypatch.setenv("UGSM_DEV", "1")
    monkeypatch.setenv("UGSM_SMALL_MASK", "0")
    monkeypatch.setenv("UGSM_ALONE", alone)
    what = f"{W}x{H}, {lv} levels, UGSM_SMALL_MASK=0, UGSM_ALONE={alone}"
    w, h = lib.level_dims(W, H, lv)
    _assert_plans_complete(lib, zip(w, h), what)
    assert lib.plan_level(w[-1], h[-1])["cost_kernel"] == 1
    L, R = _pairs(W, H, 1, 9300 + W)[0]
    with lib.Context(levels=lv, profile_events=2) as c:
        got = _full(c, [(L, R)], W, H)[0]
        _assert_every_level_ran_its_planned_cost_kernel(lib, c, W, H, lv, what, alone == "1")
    assert_bit_equal(got, orc.match_full(L, R, lv), what)


# ---- a seeded random sweep of accepted public configurations ----------------------------------------------------------------------

def _random_cases(n_cases=16, seed=2027, px_budget=6_000_000):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n_cases):
        W = int(round(np.exp(rng.uniform(np.log(48), np.log(3000)))))
        H = int(round(np.exp(rng.uniform(np.log(40), np.log(2000))))) if k % 5 else min(2000, max(40, W * 2 // 3))
        if k == 0:
            W, H = 3000, 2000
            cfg_min = int(rng.choice([m for m in MARCH_MIN if m > 6_000_000]))   # (level 0, 6 Mpx: a level only the fallback covers)
        elif k == 1:
            W, H = 48, 40
        lvmax = _max_levels(W, H)
        slots = int(rng.integers(1, 5))
        cfg = dict(march_min_pixels=int(rng.choice(MARCH_MIN)), small_max_pixels=int(rng.choice(SMALL_MAX)), batch=int(rng.choice(BATCH)),
                   slots=slots, streams=int(rng.integers(0, slots + 1)), stream_priority=int(rng.integers(0, 4)),
                   march_rows=int(rng.choice([0, 0, 7, 17, 64])))
        if k == 0:
            cfg["march_min_pixels"] = cfg_min
        foveated = k % 2 == 1 and lvmax >= 2
        lv = int(rng.integers(max(2, lvmax - 4), lvmax + 1)) if lvmax >= 2 else 1
        F = int(rng.integers(2, lv + 1)) if foveated else 0
        n = int(rng.integers(1, max(cfg["batch"], 1) + 1))
        n = max(1, min(n, px_budget // (W * H)))
        cases.append(dict(W=W, H=H, lv=lv, F=F, n=n, slot=int(rng.integers(0, slots)), cfg=cfg,
                          offs=[(int(rng.integers(-W // 2, W // 2 + 1)), int(rng.integers(-H // 2, H // 2 + 1))) for _ in range(n)],
                          blocking=bool(rng.integers(0, 2))))
    return cases


def _max_levels(W, H, most=14):
    """The pyramid levels a W x H frame has, up to `most` (matching(): w[i+1] = (int)(w[i] / 1.41421356))."""
    n = 1
    while n < most:
        W, H = int(W / 1.41421356), int(H / 1.41421356)
        if W < 1 or H < 1:
            break
        n += 1
    return n


CASES = _random_cases()


@pytest.mark.parametrize("case", CASES, ids=[f"{k}:{c['W']}x{c['H']}x{c['n']}{'F' + str(c['F']) if c['F'] else ''}" for k, c in enumerate(CASES)])
def test_random_accepted_configuration_vs_oracle(lib, orc16, case):
    """One seeded case: a public configuration drawn from the host sweep's values (plus slots, streams <= slots, stream priority, strip
    height), a frame of 48 x 40 .. 3000 x 2000, full mode (ugsm_match_full, or a ugsm_submit_full_batch call of up to `batch` pairs) or
    foveated (ugsm_submit_foveated_batch, every pair at its own offset).  The plan of every level the call runs is complete first."""
    W, H, lv, F, n, cfg = case["W"], case["H"], case["lv"], case["F"], case["n"], case["cfg"]
    what = f"{W}x{H}, {lv} levels, F={F}, {n} pair(s) on slot {case['slot']}, {cfg}"
    sizes = list(zip(*lib.level_dims(W, H, lv)))
    if F:
        sizes.append(lib.fovea_dims(W, H, lv, F))
    _assert_plans_complete(lib, sizes, what, **dict(cfg, batch=n))           # the call's own launches ...
    _assert_plans_complete(lib, sizes, what, **cfg)                          # ... and those of a call of the configured batch
    pairs = _pairs(W, H, n, 9400 + W + H)
    with lib.Context(levels=lv, fovea_levels=max(F, 2) if lv >= 2 else 0, **cfg) as c:
        if F:
            got = _foveated(c, lib, pairs, W, H, lv, F, case["offs"], slot=case["slot"])
        elif n == 1 and case["blocking"]:
            L, R = pairs[0]
            out = np.empty((3, H, W), np.float32)
            c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], out[0].ctypes.data, out[1].ctypes.data,
                                          out[2].ctypes.data))
            got = [out]
        else:
            got = _full(c, pairs, W, H, slot=case["slot"])
    for b, (L, R) in enumerate(pairs):
        exp = orc16.match_foveated(L, R, lv, F, *case["offs"][b])[0] if F else orc16.match_full(L, R, lv)
        assert_bit_equal(got[b], exp, f"{what}, pair {b}" + (f" at {case['offs'][b]}" if F else ""))


# ---- the lending slot -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pairs_1080(orc):
    pairs = _pairs(1920, 1080, 2, 9500)
    orc.set_num_threads(16)
    try:
        return pairs, [orc.match_full(L, R, 14) for L, R in pairs]
    finally:
        orc.set_num_threads(8)


@pytest.mark.parametrize("kw", [dict(slots=2), dict(slots=4, streams=2)], ids=["slots2", "slots4_streams2"])
def test_lend_a_call_on_the_lending_slot(lib, pairs_1080, kw):
    """A lone call on slot 1 forks onto slot 0's stream (ugsm_create: a slot borrows the stream of the slot before it).  Submitted at once
    behind it, a call on slot 0 -- the lender -- queues behind the borrowed work.  Both are waited for, in both orders; both results are
    the oracle's."""
    (pa, pb), (ea, eb) = pairs_1080
    W, H = 1920, 1080
    with lib.Context(levels=14, **kw) as c:
        dL = [c.to_device(p[0]) for p in (pa, pb)]
        dR = [c.to_device(p[1]) for p in (pa, pb)]
        dO = [c.alloc(3 * W * H * 4) for _ in range(2)]
        for order in ((1, 0), (0, 1)):
            c.check(c.lib.ugsm_wait_all(c.handle))                             # nothing in flight: the call on slot 1 is alone and forks
            c.check(c.lib.ugsm_submit_full(c.handle, 1, dL[0], dR[0], W, H, 3 * W, dO[0]))
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dL[1], dR[1], W, H, 3 * W, dO[1]))
            for s in order:
                c.check(c.lib.ugsm_wait(c.handle, s))
            assert_bit_equal(c.to_host(dO[0], (3, H, W)), ea, f"{kw}, waits in order {order}: the lone call on slot 1")
            assert_bit_equal(c.to_host(dO[1], (3, H, W)), eb, f"{kw}, waits in order {order}: the call on the lending slot 0")
        for p in dL + dR + dO:
            c.free(p)


def test_lend_a_call_that_fails_after_its_fork(lib, pairs_1080, monkeypatch):
    """The same with the lone call on slot 1 failing AFTER its fork: UGSM_MEM_LIMIT_MB (development) is set so that slot 1's buffers fit
    (prepare_slot) and the A planes of its side stream do not (enqueue_side_A's grow: a host-side UGSM_ERR_NOMEM, the right pyramid already
    enqueued on slot 0's stream).  Slot 0 holds all its buffers from a first call, so the lender's call needs no memory.  Slot 0's
    result is the oracle's, and ugsm_wait(1) returns, in both orders."""
    (pa, pb), (ea, eb) = pairs_1080
    W, H, lv = 1920, 1080, 14
    w, h = lib.level_dims(W, H, lv)
    apyr = 4 * sum(3 * a * b for a, b in zip(w, h))                           # A planes of every level (Slot::Apyr)

    def run(c, slot, k):
        c.check(c.lib.ugsm_submit_full(c.handle, slot, dL[k], dR[k], W, H, 3 * W, dO[k]))
        c.check(c.lib.ugsm_wait(c.handle, slot))

    with lib.Context(levels=lv, slots=2) as c:                                 # what one slot holds after a lone 1080p call
        dL, dR, dO = [c.to_device(pa[0])], [c.to_device(pa[1])], [c.alloc(3 * W * H * 4)]
        run(c, 0, 0)
        one_slot = c.device_bytes()
        for p in dL + dR + dO:
            c.free(p)
    assert one_slot > apyr, (one_slot, apyr)
    limit = one_slot + (one_slot - apyr) + apyr // 2                          # slot 0 whole, slot 1 without its A planes, half of them
    monkeypatch.setenv("UGSM_DEV", "1")
    monkeypatch.setenv("UGSM_MEM_LIMIT_MB", str(limit >> 20))
    with lib.Context(levels=lv, slots=2) as c:
        dL = [c.to_device(p[0]) for p in (pa, pb)]
        dR = [c.to_device(p[1]) for p in (pa, pb)]
        dO = [c.alloc(3 * W * H * 4) for _ in range(2)]
        run(c, 0, 1)                                                           # slot 0's buffers, A planes included
        assert c.device_bytes() == one_slot
        assert_bit_equal(c.to_host(dO[1], (3, H, W)), eb, "slot 0 alone under the limit")
        for order in ((1, 0), (0, 1)):
            c.check(c.lib.ugsm_wait_all(c.handle))
            st = c.lib.ugsm_submit_full(c.handle, 1, dL[0], dR[0], W, H, 3 * W, dO[0])
            assert st == lib.UGSM_ERR_NOMEM, (order, st, c.lib.ugsm_last_error(c.handle))
            assert b"hipMalloc" in c.lib.ugsm_last_error(c.handle)
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dL[1], dR[1], W, H, 3 * W, dO[1]))
            for s in order:
                assert c.lib.ugsm_wait(c.handle, s) == lib.UGSM_OK, (order, s, c.lib.ugsm_last_error(c.handle))
            assert_bit_equal(c.to_host(dO[1], (3, H, W)), eb, f"the lending slot 0 beside a failed lone call on slot 1, waits in order {order}")
        assert c.device_bytes() <= limit
        for p in dL + dR + dO:
            c.free(p)
