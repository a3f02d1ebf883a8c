#!/usr/bin/env python3
"""Rewrites CUDA kernel launches so that a C++ compiler without CUDA support can parse the file.

    K<<<grid, block>>>(args);   ->   cpu_launch(grid, block, [&]{ K(args); });

Kernels (`__global__ void K(...)`) whose text calls __syncthreads() are launched with cpu_launch_sync, which runs the
threads of a block as real threads (oracle/ref_cpu/cuda_runtime.h).  Nothing else in the file changes, so line numbers stay.
The output is a build product: it goes where the caller says (oracle/_ref/), never into the tree.

    launch_rewrite.py IN.cu OUT.cpp
"""
import re
import sys

LAUNCH = re.compile(r"(\b\w+)\s*<<<\s*([^,<>]+?)\s*,\s*([^,<>]+?)\s*>>>\s*\(([^;]*?)\)\s*;", re.S)
KERNEL = re.compile(r"__global__\s+void\s+(\w+)\s*\(")


def kernels_with_barriers(text):
    heads = list(KERNEL.finditer(text))
    sync = set()
    for k, m in enumerate(heads):
        end = heads[k + 1].start() if k + 1 < len(heads) else len(text)
        nxt = text.find('extern "C"', m.end())
        if nxt != -1:
            end = min(end, nxt)
        if "__syncthreads" in text[m.end():end]:
            sync.add(m.group(1))
    return sync


def rewrite(text):
    sync = kernels_with_barriers(text)
    seen = []

    def sub(m):
        name, grid, block, args = m.groups()
        seen.append(name)
        # the replacement keeps the launch's line count
        pad = "\n" * (m.group(0).count("\n") - args.count("\n"))
        fn = "cpu_launch_sync" if name in sync else "cpu_launch"
        return f"{fn}({grid}, {block}, [&]{{ {name}({args}); }});{pad}"
    out = LAUNCH.sub(sub, text)
    if "<<<" in out or ">>>" in out:
        raise SystemExit("launch_rewrite: a launch was not recognised")
    return out, seen, sync


if __name__ == "__main__":
    src, dst = sys.argv[1], sys.argv[2]
    with open(src, encoding="utf-8", errors="replace") as f:
        out, seen, sync = rewrite(f.read())
    with open(dst, "w", encoding="utf-8") as f:
        f.write(out)
    print(f"launch_rewrite: {len(seen)} launches, {len([k for k in seen if k in sync])} with barriers -> {dst}")
