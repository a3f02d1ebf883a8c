#!/usr/bin/env python3
"""Writes tests/golden/launch_census.json: the launch census (tests/launch_census.py) of every case, taken on the MI355X.

Run it on a build of the commit a refactoring of the call-sequencing code STARTS from, never on the code under test:

    python tests/golden/make_launch_census.py [--out FILE] [--commit ID]

The libraries of the tree the script lies in are used as they are built (make -C ug_stereomatcher_amd/csrc); --commit names the commit in the
file (default: git's HEAD of that tree)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["UGSM_DEV"] = "1"   # (the development overrides of the policies are read only under it, as tests/conftest.py sets it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "launch_census.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    import launch_census as lc
    from ug_stereomatcher_amd import _lib
    commit = a.commit
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    cases = {}
    for policy, case in lc.case_ids():
        cases[f"{policy}/{case}"] = lc.census(_lib, policy, case)
        print(f"{policy}/{case}: {len(cases[f'{policy}/{case}']['launches'])} (kernel, level) cells", flush=True)
    doc = {"commit": commit, "size": [lc.W, lc.H], "levels": lc.LEVELS, "fovea_levels": lc.F, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {a.out}: {len(cases)} cases at commit {commit}")


if __name__ == "__main__":
    main()
