"""Host-only sweep of the configuration space (ugsm_plan_level; no GPU needed): for every ugsm_config that ugsm_create in libugsm.so
accepts, every level of every call must run a K-cost kernel the library ships.  The sizes sit on and around every kernel-choice threshold,
compared with what one launch holds (pairs x W x H), and on the levels of the frames the suite and the node use.

A level that no form covers used to fall through to the development library's LDS-tiled k_cost_split, whose stand-in in libugsm.so
launches nothing: every iteration's cost step was skipped and the call still answered UGSM_OK.  The policy functions now give such a
level to k_cost_march, and these tests pin that for the public fields, for the development overrides, and for the agreement of
ugsm_plan_level with ugsm_create (a plan is never reported for a configuration no context can have)."""
import ctypes as C
import itertools

import pytest

from ug_stereomatcher_amd import _lib

TILED, MARCH, SMALL, STAGED, MARCH4 = 0, 1, 2, 3, 4
MARCHING = (MARCH, MARCH4)
K_BATCH_MAX_PIXELS = 9_000_000          # kBatchMaxPixels (ugsm_policy.cpp): levels up to here are one launch for all pairs of a batched call
THRESHOLDS = (50_000, 150_000, 400_000, 3_000_000, K_BATCH_MAX_PIXELS)   # the shared / alone latency reach, the marching default, k_cost_march4's top

MARCH_MIN = (0, 1, 49_999, 50_000, 150_000, 400_000, 3_000_000, 3_000_001, 10**7, 2**28, 2**31 - 1)
SMALL_MAX = (-1, 0, 1, 50_000, 150_000, 3 * 10**6, 10**9)
BATCH = (0, 1, 2, 3, 8, 16)
MARCH_ROWS = (0, 17)
FRAMES = ((4928, 3264), (1920, 1080), (640, 480), (160, 120), (3000, 2000), (2600, 1700), (2828, 2828), (2000, 2000))


def _frame_levels():
    out = set()
    for W, H in FRAMES:
        for lv in range(14, 0, -1):          # as many levels as the frame has (160 x 120: 12)
            try:
                w, h = _lib.level_dims(W, H, lv)
            except _lib.UgsmError:
                continue
            out.update(zip(w, h))
            break
    return out


def _near_square(n):
    """A W x H with W * H == n exactly, as square as the divisors of n allow."""
    h = int(n ** 0.5)
    while n % h:
        h -= 1
    return (n // h, h)


def level_sizes(batch):
    """The frames' levels, and levels whose pixel count -- alone or times the pairs of a call of `batch` -- is one below, at and one
    above each threshold."""
    pairs = max(batch, 1)
    px = set()
    for t in THRESHOLDS:
        px.update((t - 1, t, t + 1))
        if pairs > 1:
            px.update(((t - 1) // pairs, t // pairs, -(-t // pairs), -(-(t + 1) // pairs)))
    return sorted(_frame_levels() | {_near_square(n) for n in px if n >= 1})


class Planner:
    """ugsm_plan_level on one library, without the per-call overhead of _lib.plan_level (the sweep asks a few hundred thousand times)."""

    def __init__(self, dev=False):
        self.lib = _lib.load(dev)
        self.out = _lib.LevelPlan()

    def config(self, **fields):
        cfg = _lib.Config()
        self.lib.ugsm_default_config(C.byref(cfg))
        for k, v in fields.items():
            setattr(cfg, k, v)
        return cfg

    def plan(self, cfg, alone, W, H):
        st = self.lib.ugsm_plan_level(C.byref(cfg), 1 if alone else 0, W, H, C.byref(self.out))
        return st, {k: getattr(self.out, k) for k, _ in _lib.LevelPlan._fields_}

    def create_status(self, cfg):
        """ugsm_create's answer (a context it makes is destroyed at once)."""
        h = C.c_void_p()
        st = self.lib.ugsm_create(C.byref(cfg), C.byref(h))
        if h.value:
            self.lib.ugsm_destroy(h)
        return st


def plan_problems(p, W, H, batch):
    """What is incomplete about the plan of a W x H level (empty: nothing)."""
    bad = []
    cost = p["cost_kernel"]
    if cost not in (MARCH, SMALL, MARCH4):
        bad.append(f"cost_kernel {cost}")
    if (p["strip_rows"] > 0) != (cost in MARCHING):
        bad.append(f"strip_rows {p['strip_rows']} with cost_kernel {cost}")
    if p["smooth_kernel"] not in (TILED, SMALL) or p["smooth_rh"] not in (0, 18, 24, 32) or \
            (p["smooth_kernel"] == SMALL) != (p["smooth_rh"] in (18, 24, 32)):
        bad.append(f"smooth_kernel {p['smooth_kernel']} with smooth_rh {p['smooth_rh']}")
    if p["seed_fused"] and cost not in MARCHING:
        bad.append(f"seed_fused on cost_kernel {cost}")
    if not p["seed_fused"] and cost in MARCHING:      # (UGSM_FUSE_SEED and early_exit_threshold stay at their defaults here)
        bad.append(f"marching cost_kernel {cost} without the fused seeding")
    want = max(batch, 1) if W * H <= K_BATCH_MAX_PIXELS else 1
    if p["pairs_per_launch"] != want:
        bad.append(f"pairs_per_launch {p['pairs_per_launch']} (want {want})")
    return bad


def _report(failures, what):
    if failures:
        head = "\n".join(failures[:60])
        more = f"\n... and {len(failures) - 60} more" if len(failures) > 60 else ""
        pytest.fail(f"{len(failures)} incomplete plans {what}:\n{head}{more}", pytrace=False)


def sweep(planner, grid, refused=None):
    """Plans every level size of every configuration in `grid` (dicts of ugsm_config fields); returns the failing cells.  A configuration
    whose first plan answers UGSM_ERR_BAD_ARG is collected in `refused` when that is given (and not planned further), a failure otherwise."""
    failures = []
    sizes = {}
    for fields in grid:
        batch = fields.get("batch", 0)
        if batch not in sizes:
            sizes[batch] = level_sizes(batch)
        cfg = planner.config(**fields)
        name = ", ".join(f"{k}={v}" for k, v in fields.items())
        if refused is not None and planner.plan(cfg, True, *sizes[batch][0])[0] == _lib.UGSM_ERR_BAD_ARG:
            refused.append(name)
            continue
        for alone, (W, H) in itertools.product((True, False), sizes[batch]):
            st, p = planner.plan(cfg, alone, W, H)
            if st != _lib.UGSM_OK:
                failures.append(f"[{name}, alone={alone}] {W}x{H}: ugsm_plan_level status {st}")
                continue
            bad = plan_problems(p, W, H, batch)
            if bad:
                pairs = max(batch, 1) if W * H <= K_BATCH_MAX_PIXELS else 1
                failures.append(f"[{name}, alone={alone}] {W}x{H} ({W * H * pairs} px per launch): {'; '.join(bad)}")
    return failures


def public_grid():
    for mm, sm, b, rows in itertools.product(MARCH_MIN, SMALL_MAX, BATCH, MARCH_ROWS):
        yield dict(march_min_pixels=mm, small_max_pixels=sm, batch=b, march_rows=rows)


@pytest.fixture
def no_dev_overrides(monkeypatch):
    """The public fields alone: no development override of this process acts (UGSM_DEV unset)."""
    monkeypatch.delenv("UGSM_DEV", raising=False)


def test_every_level_of_every_accepted_public_configuration_runs_a_shipped_cost_kernel(no_dev_overrides):
    planner = Planner()
    _report(sweep(planner, public_grid()), "on libugsm.so")


def test_the_default_configuration_never_needs_the_fallback(no_dev_overrides):
    """With the default thresholds the shipped forms cover every size by themselves: k_cost_march stays where it was (>= 0.4 Mpx per launch
    and above k_cost_march4's reach), so that no default plan changed when the fallback came."""
    planner = Planner()
    for batch in BATCH:
        cfg = planner.config(batch=batch)
        for alone in (True, False):
            for W, H in level_sizes(batch):
                st, p = planner.plan(cfg, alone, W, H)
                px = W * H * p["pairs_per_launch"]
                small_max = 150_000 if alone else 50_000
                want = SMALL if px <= small_max else (MARCH4 if px <= 3_000_000 else MARCH)
                assert st == _lib.UGSM_OK and p["cost_kernel"] == want, (batch, alone, W, H, p)


# the development overrides the tests and tools steer the kernel choice with (read under UGSM_DEV=1 only, by ugsm_create and ugsm_plan_level alike)
DEV_ENV = [dict(zip(("UGSM_SMALL_MASK", "UGSM_MARCH4", "UGSM_MARCH_MIN_PIXELS"), v))
           for v in itertools.product(("0", "1", "2", "3", None), ("0,0", "1,100000", None), (None, "1", "10000000", "2147483647", "-1"))]


@pytest.mark.parametrize("env", DEV_ENV, ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items() if v is not None) or "none")
def test_every_level_under_the_development_overrides_runs_a_shipped_cost_kernel(monkeypatch, env):
    """The same invariant on libugsm.so under UGSM_SMALL_MASK (k_cost_small / k_smooth_small switched off in turn), UGSM_MARCH4 (k_cost_march4
    never, or on a range of its own) and UGSM_MARCH_MIN_PIXELS -- unless ugsm_create refuses the configuration, which ugsm_plan_level must
    then refuse as well (UGSM_MARCH_MIN_PIXELS=-1: the tiled K-cost is libugsm_dev.so's)."""
    monkeypatch.setenv("UGSM_DEV", "1")
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    planner = Planner()
    grid = [dict(march_min_pixels=mm, small_max_pixels=sm, batch=b)
            for mm, sm, b in itertools.product((0, 10**7), (-1, 0, 10**9), (1, 8))]
    refused = []
    failures = sweep(planner, grid, refused=refused)
    if env["UGSM_MARCH_MIN_PIXELS"] == "-1":
        assert len(refused) == len(grid) and not failures, (refused, failures[:10])
        for fields in grid:
            assert planner.create_status(planner.config(**fields)) == _lib.UGSM_ERR_BAD_ARG, fields
    else:
        assert not refused, refused
    _report(failures, f"on libugsm.so under {env}")


def test_the_fallback_cells_march():
    """The cells that had no K-cost in libugsm.so: k_cost_march takes them, with its strip height and the fused seeding."""
    cells = [
        (3484, 2307, dict(march_min_pixels=10_000_000)), (2463, 1631, dict(march_min_pixels=2**31 - 1)),   # levels 1, 2 of 16 MP
        (2828, 2828, dict(march_min_pixels=10_000_000)), (2000, 2000, dict(march_min_pixels=10_000_000)),
        (3000, 2000, dict(march_min_pixels=10_000_000)),
        (1920, 1080, dict(march_min_pixels=2**31 - 1, batch=2)),                                          # 4.1 Mpx per launch
        (640, 480, dict(march_min_pixels=2**31 - 1, batch=16)), (615, 407, dict(march_min_pixels=2**31 - 1, batch=16)),   # 4.9 / 4.0 Mpx
        (870, 576, dict(march_min_pixels=2**31 - 1, batch=8)), (959, 539, dict(march_min_pixels=2**31 - 1, batch=8)),     # 4.0 / 4.1 Mpx
    ]
    for W, H, fields in cells:
        for alone in (True, False):
            p = _lib.plan_level(W, H, alone=alone, **fields)
            assert p["cost_kernel"] == MARCH and p["strip_rows"] > 0 and p["seed_fused"] == 1, (W, H, fields, alone, p)
    # where march_min_pixels puts the threshold in k_cost_march4's range, k_cost_march4 still comes first (asked first, as before)
    assert _lib.plan_level(1741, 1153, march_min_pixels=10_000_000)["cost_kernel"] == MARCH4


# ---- ugsm_plan_level and ugsm_create agree ---------------------------------------------------------------------------------------------

AGREEMENT = [   # (ugsm_config fields, development environment)
    ({}, {}),
    (dict(march_min_pixels=2**31 - 1, batch=16), {}),
    (dict(small_max_pixels=-1, march_rows=5, slots=6, streams=1, stream_priority=3), {}),
    (dict(levels=1, fovea_levels=0), {}),
    (dict(levels=32, fovea_levels=32), {}),
    (dict(levels=0), {}),
    (dict(levels=33), {}),
    (dict(slots=0), {}),
    (dict(slots=65), {}),
    (dict(kernel_path=1), {}),
    (dict(kernel_path=2), {}),
    (dict(kernel_path=-1), {}),
    (dict(march_min_pixels=-1), {}),
    (dict(fovea_levels=15), {}),
    (dict(fovea_levels=-1), {}),
    (dict(lr_check_threshold=-0.5), {}),
    (dict(lr_check_threshold=float("nan")), {}),
    (dict(streams=-1), {}),
    (dict(batch=-1), {}),
    (dict(batch=17), {}),
    (dict(stream_priority=4), {}),
    (dict(stream_priority=-1), {}),
    ({}, {"UGSM_KERNEL_PATH": "1"}),
    ({}, {"UGSM_MARCH_MIN_PIXELS": "-1"}),
    (dict(kernel_path=1), {"UGSM_KERNEL_PATH": "0"}),
    (dict(march_min_pixels=-1), {"UGSM_MARCH_MIN_PIXELS": "0"}),
]


@pytest.mark.parametrize("dev", [False, True], ids=["libugsm", "libugsm_dev"])
def test_plan_refuses_exactly_what_create_refuses(monkeypatch, dev):
    """ugsm_plan_level answers UGSM_ERR_BAD_ARG for every configuration -- after the development overrides -- that ugsm_create in the same
    library refuses, and plans every one it accepts.  Accepted: UGSM_OK where there is a device (the context is destroyed at once), any
    answer but UGSM_ERR_BAD_ARG where there is none (ugsm_create then stops at UGSM_ERR_NO_DEVICE, past the validation)."""
    planner = Planner(dev)
    seen = set()
    for fields, env in AGREEMENT:
        monkeypatch.setenv("UGSM_DEV", "1")
        for k in ("UGSM_KERNEL_PATH", "UGSM_MARCH_MIN_PIXELS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cfg = planner.config(**fields)
        created = planner.create_status(cfg)
        assert created in (_lib.UGSM_OK, _lib.UGSM_ERR_BAD_ARG, _lib.UGSM_ERR_NO_DEVICE), (fields, env, created)
        seen.add(created)
        planned, _ = planner.plan(cfg, True, 640, 480)
        what = f"{'libugsm_dev' if dev else 'libugsm'} {fields} under {env}: ugsm_create {created}, ugsm_plan_level {planned}"
        if created == _lib.UGSM_ERR_BAD_ARG:
            assert planned == _lib.UGSM_ERR_BAD_ARG, what
        else:
            assert planned == _lib.UGSM_OK, what
    assert not ({_lib.UGSM_OK, _lib.UGSM_ERR_NO_DEVICE} <= seen), "a device that comes and goes"
    assert _lib.UGSM_ERR_BAD_ARG in seen
