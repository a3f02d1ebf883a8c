"""The slot's memory types (csrc/ugsm_mem.hpp: MemBook, DevBuf, GroupCap, PinnedBuf, UploadRing) on a machine without a GPU:
tests/slot_mem_sanitize.cpp -- its own main, the header, malloc-backed stand-ins for the runtime calls it uses -- built with
-fsanitize=address,undefined and run as a program of its own (nothing is loaded into Python).

What the program asserts: a growth frees before it allocates and a smaller need allocates nothing; the book equals the live counted
allocations after every step and an uncounted buffer never moves it; a group of 2, 3 or 5 buffers whose growth fails at any member holds
nothing, at capacity 0, and grows later; the ring's copies take turns, a turn waits for its own previous upload alone, a growth drops the
recorded uploads, an upload copies exactly its rows; after the releases nothing is live."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")


def test_the_header_needs_nothing_of_the_project():
    """ugsm_mem.hpp includes the HIP runtime API and the standard library only: the program above compiles it without the launch or
    kernel headers."""
    with open(os.path.join(CSRC, "ugsm_mem.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert [i for i in includes if "hip" in i] == ["<hip/hip_runtime_api.h>"], includes


def test_the_memory_types_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "slot_mem_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "slot_mem_sanitize.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ok:" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
