"""The launch census of every call mode against the one recorded at the commit named in tests/golden/launch_census.json.

What a census is and how it is taken: tests/launch_census.py.  The golden file is written by tests/golden/make_launch_census.py on a build
of that commit; here the code under test has to launch the same kernels, on the same levels, the same number of times and in the same
groups, and write the same bytes, case by case."""
import json
import os

import pytest

import launch_census as lc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "launch_census.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def test_the_golden_file_lists_the_cases():
    assert (RECORDED["size"], RECORDED["levels"], RECORDED["fovea_levels"]) == ([lc.W, lc.H], lc.LEVELS, lc.F)
    assert list(RECORDED["cases"]) == [f"{p}/{k}" for p, k in lc.case_ids()]
    assert all(r["launches"] and r["sha256"] for r in RECORDED["cases"].values())


@pytest.mark.parametrize("policy,case", lc.case_ids(), ids=[f"{p}/{k}" for p, k in lc.case_ids()])
def test_launch_census(lib, policy, case):
    want = RECORDED["cases"][f"{policy}/{case}"]
    got = lc.census(lib, policy, case)
    rows = [list(r) for r in got["launches"]]
    for r in sorted(map(tuple, rows + want["launches"])):   # what differs, readably, before the whole lists are compared
        if (list(r) in rows) != (list(r) in want["launches"]):
            print(("only now:      " if list(r) in rows else "only recorded: ") + str(r))
    assert rows == want["launches"], f"{policy}/{case}: the launches differ from those recorded at {RECORDED['commit']}"
    assert got["sha256"] == want["sha256"], f"{policy}/{case}: an output buffer differs from the one recorded at {RECORDED['commit']}"
