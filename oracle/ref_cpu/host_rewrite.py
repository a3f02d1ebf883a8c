#!/usr/bin/env python3
"""Writes the copy of the reference's host driver that is compiled for the CPU, with one change: the stack arrays that the driver
overruns are made large enough.

    every array bound [MAX_LEVEL-1]   ->   [MAX_LEVEL+1]

CreateFoveatedPyramid and initStack declare their per-level height and width arrays with MAX_LEVEL - 1 ints and store up to index MAX_LEVEL; where those stores land is
the compiler's choice (with the stack protector on, the program aborts).  MAX_LEVEL + 1 elements hold every index that is stored, and
the values stored and read stay what they were.  Nothing else in the file changes, so line numbers stay.  The output is a build product:
it goes where the caller says (oracle/_ref/), never into the tree.

    host_rewrite.py IN.cpp OUT.cpp
"""
import re
import sys

SHORT = re.compile(r"\[\s*MAX_LEVEL\s*-\s*1\s*\]")


def rewrite(text):
    return SHORT.subn("[MAX_LEVEL+1]", text)


if __name__ == "__main__":
    src, dst = sys.argv[1], sys.argv[2]
    with open(src, encoding="utf-8", errors="replace") as f:
        out, n = rewrite(f.read())
    if n == 0:
        raise SystemExit("host_rewrite: no array of MAX_LEVEL-1 elements found")
    with open(dst, "w", encoding="utf-8") as f:
        f.write(out)
    print(f"host_rewrite: {n} array bounds enlarged -> {dst}")
