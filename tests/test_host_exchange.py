"""The rank-order sum through shared memory (csrc/host_exchange.h) without a GPU: tests/host_exchange_driver.cpp, built
with the address and undefined-behaviour sanitizers, forks the ranks and prints every rank's result of every round as
hex doubles (the 16 hex digits of each double's bit pattern); the sums are compared here, bit for bit, with NumPy's
left-to-right sum in rank order starting from 0.0."""
import glob
import itertools
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "vlgp_amd", "csrc")
SMALL, LARGE = 64, 1 << 17          # slot capacities of the H-step exchange and of the test transport
PREFIX = {SMALL: "/vlgp_hx_", LARGE: "/vlgp_shm_"}
PATTERN = (1e16, 1.0, -1e16)        # order-sensitive: (1e16 + 1) - 1e16 = 0, (1e16 - 1e16) + 1 = 1
_ids = itertools.count()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_exchange") / "host_exchange_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "host_exchange_driver.cpp"), "-o", exe, "-lrt"],
                   check=True, timeout=300)
    return exe


def _run(exe, world, policy, cap, ns, timeout_s=30.0, missing=-1, limit=120):
    """Run the driver; {"name": segment, "rounds": {(rank, round): (seq, "ok", bits) or (seq, "err", what)}, "seconds"}."""
    uid = "t-%d-%d-%d" % (os.getpid(), next(_ids), time.time_ns())
    t0 = time.time()
    done = subprocess.run([exe, PREFIX[cap], uid, str(world), policy, str(cap), str(timeout_s), str(missing)]
                          + [str(n) for n in ns], capture_output=True, timeout=limit)
    seconds = time.time() - t0
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    out = {"name": None, "rounds": {}, "seconds": seconds}
    for ln in done.stdout.decode().splitlines():
        f = ln.split(" ")
        if f[0] == "name":
            out["name"] = f[1]
            continue
        assert f[0] == "rank" and f[2] == "round" and f[4] == "seq", ln[:80]
        key, seq = (int(f[1]), int(f[3])), int(f[5])
        if f[6] == "ok":
            out["rounds"][key] = (seq, "ok", np.frombuffer(bytes.fromhex(f[7] if len(f) > 7 else ""), dtype=">u8"))
        else:
            out["rounds"][key] = (seq, "err", " ".join(f[7:]))
    assert out["name"] and out["name"].startswith(PREFIX[cap])
    return out


def _reference_bits(world, n, r):
    """NumPy, left to right in rank order from 0.0, of what the driver's ranks contribute in round r."""
    scale = (1 + np.arange(n) + r).astype(np.float64)
    total = np.zeros(n)
    for k in range(world):
        total = total + PATTERN[k % 3] * scale
    return total.view(np.uint64)


def _gone(name):
    return not os.path.exists("/dev/shm" + name) and not glob.glob("/dev/shm/vlgp_*" + name.rsplit("_", 1)[1])


def _lengths(cap):
    """50 rounds, another length each: the corner lengths first, then lengths spread over the region."""
    first = [0, 1, 63, 64] if cap == SMALL else [1, 1000, cap]
    step, span = (37, SMALL + 1) if cap == SMALL else (7919, 3001)
    return first + [(r * step) % span for r in range(len(first), 50)]


@pytest.mark.parametrize("cap", [SMALL, LARGE], ids=["slots64", "slots128k"])
@pytest.mark.parametrize("policy", ["sleep", "spin"])
@pytest.mark.parametrize("world", [1, 2, 3, 16])
def test_rank_order_sum_is_bit_identical_on_every_rank(driver, world, policy, cap):
    ns = _lengths(cap)
    assert len(ns) == 50 and max(ns) == cap
    got = _run(driver, world, policy, cap, ns)
    assert sorted(got["rounds"]) == [(k, r) for k in range(world) for r in range(50)]
    for r, n in enumerate(ns):
        want = _reference_bits(world, n, r)
        for k in range(world):
            seq, what, bits = got["rounds"][(k, r)]
            assert (seq, what) == (r + 1, "ok") and bits.size == n, (k, r, seq, what)
            assert np.array_equal(bits.astype(np.uint64), want), (k, r, n)
    if world == 3:  # the inputs do tell the orders apart: ranks 0, 1, 2 give 0.0, ranks 0, 2, 1 would give 1.0
        assert _reference_bits(3, 1, 0)[0] == 0 and (PATTERN[0] + PATTERN[2]) + PATTERN[1] == 1.0
    assert _gone(got["name"])


@pytest.mark.parametrize("cap", [SMALL, LARGE], ids=["slots64", "slots128k"])
@pytest.mark.parametrize("policy", ["sleep", "spin"])
def test_a_length_above_the_capacity_is_refused_and_touches_nothing(driver, policy, cap):
    got = _run(driver, 3, policy, cap, [5, cap + 1, -1, 5])
    for k in range(3):
        assert got["rounds"][(k, 0)][:2] == (1, "ok")
        assert got["rounds"][(k, 1)] == (1, "err", "size") and got["rounds"][(k, 2)] == (1, "err", "size")  # no round begun
        seq, what, bits = got["rounds"][(k, 3)]                                                          # ... the next is round 2
        assert (seq, what) == (2, "ok") and np.array_equal(bits.astype(np.uint64), _reference_bits(3, 5, 3))
    assert _gone(got["name"])


@pytest.mark.parametrize("cap", [SMALL, LARGE], ids=["slots64", "slots128k"])
@pytest.mark.parametrize("policy", ["sleep", "spin"])
def test_a_missing_rank_is_named_and_nothing_hangs(driver, policy, cap):
    got = _run(driver, 3, policy, cap, [4, 4], timeout_s=0.3, missing=1, limit=20)
    assert sorted(got["rounds"]) == [(0, 0), (2, 0)]  # the ranks stop at the first round
    for k in (0, 2):
        assert got["rounds"][(k, 0)] == (1, "err", "rank 1")
    assert got["seconds"] < 3.0  # 0.3 s of waiting; the rest is starting three sanitized processes
    assert _gone(got["name"])
