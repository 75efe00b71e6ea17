"""The owners of device memory (csrc/dev_mem.h) without a GPU: tests/dev_mem_driver.cpp supplies malloc-backed stand-ins
for the seven HIP calls the header names and is built with the address and undefined-behaviour sanitizers, so a block
freed twice, used after its release or never freed ends the case.  Each case also checks that it made one free per block
it was handed and left the four live-memory counters at zero.  Last, a search of the sources: nothing but the header
allocates or frees."""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "vlgp_amd", "csrc")
CASES = (
    "freed_once_by_destruction", "freed_once_by_reset", "freed_once_by_second_alloc", "freed_once_by_move_assignment",
    "borrowed_never_freed", "moved_from_is_empty", "failed_alloc_leaves_empty", "ensure_within_len_makes_no_call",
    "ensure_allocates_the_capacity", "ensure_synchronises_with_a_stream_only", "failed_growth_leaves_empty",
    "host_blocks_and_handles",
)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dev_mem") / "dev_mem_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "dev_mem_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_driver_has_these_cases(driver):
    done = subprocess.run([driver, "list"], capture_output=True, timeout=60)
    assert done.returncode == 0 and tuple(done.stdout.decode().split()) == CASES


@pytest.mark.parametrize("case", CASES)
def test_owner(driver, case):
    done = subprocess.run([driver, case], capture_output=True, timeout=60)
    out = done.stdout.decode(errors="replace") + done.stderr.decode(errors="replace")
    assert done.returncode == 0 and done.stdout.decode().strip() == "ok", out[-3000:]


def test_only_the_header_allocates_and_frees():
    calls = re.compile(r"\b(hipFree|hipHostFree|hipMalloc|hipHostMalloc)\(")
    seen = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path) or path.endswith(".o"):  # (every source, the Makefile too; not a build's objects)
            continue
        with open(path, errors="replace") as f:
            hits = sorted(set(calls.findall(f.read())))
        if hits:
            seen[os.path.basename(path)] = hits
    assert seen == {"dev_mem.h": ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"]}
