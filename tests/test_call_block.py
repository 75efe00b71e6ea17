"""The device-block layouts of the six scoring entry points (csrc/call_block.h) without a GPU: tests/call_block_driver.cpp,
built with the address and undefined-behaviour sanitizers, prints every region's offset and the block's size; here they
are compared with the offset chains the entry points carried before the layouts were functions (written out below as
plain arithmetic, offsets in doubles), and the regions are checked to lie in order, without overlap, up to ``need``."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "vlgp_amd", "csrc")
I64 = {"tab"}                                      # regions read as int64_t
SHAPES = {                                         # unit lengths, L, R, N
    "ones": ([1], 1, 1, 1),                        # M = L = R = rows = 1: one task (odd)
    "even": ([1, 7], 2, 2, 3),                     # 4 tasks (even)
    "ragged": ([1, 7, 65], 3, 4, 5),               # 9 tasks (odd), more than one row tile per unit
}
TILE_ROWS = 32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("call_block") / "call_block_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tests", "call_block_driver.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _run(exe, call, *args):
    done = subprocess.run([exe, call] + [str(int(a)) for a in args], capture_output=True, timeout=60)
    assert done.returncode == 0, done.stderr.decode(errors="replace")[-3000:]
    pairs = [ln.split(" ") for ln in done.stdout.decode().splitlines()]
    assert pairs and pairs[-1][0] == "need"
    return [(k, int(v)) for k, v in pairs]


def _dims(shape):
    lengths, L, R, N = SHAPES[shape]
    M, rows = len(lengths), sum(lengths)
    n_tiles = sum((T + TILE_ROWS - 1) // TILE_ROWS for T in lengths)
    return lengths, L, R, N, M, rows, M * L, n_tiles, (rows + 255) // 256


def _check(got, want, sizes):
    """got: the driver's (region, offset) pairs and ("need", total); want: the same from the old chains; sizes: doubles
    per region, from the shapes the launchers document."""
    assert got == want
    names, offs = [k for k, _ in got[:-1]], [o for _, o in got[:-1]]
    need = got[-1][1]
    assert names == list(sizes) and offs[0] == 0
    for i, name in enumerate(names):
        end = offs[i] + sizes[name]
        assert sizes[name] >= 0 and end <= (offs[i + 1] if i + 1 < len(offs) else need), (name, offs, need)
        if name in I64:
            assert (offs[i] * 8) % 8 == 0  # offsets count doubles off a hipMalloc'ed base
    last = names[-1]
    assert offs[-1] + sizes[last] == need


def _sample_sizes(M, L, R, tasks, n_tiles, k):
    return {"eps": tasks * R * k, "beta": tasks * R * k, "c": tasks * k, "part": n_tiles * k, "lw": M * k, "parts": M * 2 * k,
            "tab": M + 1}


@pytest.mark.parametrize("want_rate", [False, True])
@pytest.mark.parametrize("replicas", [0, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_loglik_layout(driver, shape, replicas, want_rate):
    _, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    slots, n_rate = (replicas * N if replicas else N), rows * N
    o_sums = n_rate if want_rate else 0
    need = o_sums + 4 * slots
    want = [("rate", 0), ("sums", o_sums), ("need", need)]
    _check(_run(driver, "loglik", slots, n_rate, want_rate), want, {"rate": n_rate if want_rate else 0, "sums": 4 * slots})


@pytest.mark.parametrize("want_lpd", [False, True])
@pytest.mark.parametrize("want_rate", [False, True])
@pytest.mark.parametrize("replicas", [0, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_predictive_layout(driver, shape, replicas, want_rate, want_lpd):
    _, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    slots, n_rate = (replicas * N if replicas else N), rows * N
    o_rate = 128
    o_lpd = o_rate + (n_rate if want_rate else 0)
    o_sums = o_lpd + (n_rate if want_lpd else 0)
    o_part = o_sums + 4 * slots
    need = o_part + slots * n_blk * 4
    want = [("nodes", 0), ("rate", o_rate), ("lpd", o_lpd), ("sums", o_sums), ("part", o_part), ("need", need)]
    sizes = {"nodes": 128, "rate": n_rate if want_rate else 0, "lpd": n_rate if want_lpd else 0, "sums": 4 * slots,
             "part": slots * n_blk * 4}
    _check(_run(driver, "predictive", slots, n_rate, n_blk, want_rate, want_lpd), want, sizes)


@pytest.mark.parametrize("want_rows", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_elbo_layout(driver, shape, want_rows):
    _, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    o_sums = N * n_blk * 4
    o_terms = o_sums + 4 * N
    o_rows = o_terms + 4 * tasks
    o_flag = o_rows + (rows if want_rows else 0)
    need = o_flag + (tasks + 1) // 2
    want = [("part", 0), ("sums", o_sums), ("terms", o_terms), ("rows", o_rows), ("flag", o_flag), ("need", need)]
    sizes = {"part": N * n_blk * 4, "sums": 4 * N, "terms": 4 * tasks, "rows": rows if want_rows else 0,
             "flag": (tasks + 1) // 2}  # two int flags per double
    _check(_run(driver, "elbo", rows, N, tasks, n_blk, want_rows), want, sizes)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_forecast_layout(driver, shape):
    lengths, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    n_ext = {T: 2 + i for i, T in enumerate(sorted(set(lengths)))}
    g_len = sum(L * k * R for k in n_ext.values())
    n_out = sum(n_ext[T] for T in lengths) * L
    o_g = rows * L
    o_mu = o_g + g_len
    o_v = o_mu + n_out
    o_terms = o_v + n_out
    o_tab = o_terms + 2 * tasks
    o_flag = o_tab + (2 * M + 1)
    need = o_flag + (tasks + 1) // 2
    want = [("z", 0), ("g", o_g), ("mu", o_mu), ("v", o_v), ("terms", o_terms), ("tab", o_tab), ("flag", o_flag),
            ("need", need)]
    sizes = {"z": rows * L, "g": g_len, "mu": n_out, "v": n_out, "terms": 2 * tasks, "tab": 2 * M + 1,
             "flag": (tasks + 1) // 2}
    _check(_run(driver, "forecast", rows, L, M, g_len, n_out), want, sizes)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_marginal_layout(driver, shape):
    _, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    o_eps = rows * L
    o_beta = o_eps + tasks * R * 64
    o_c = o_beta + tasks * R * 64
    o_part = o_c + tasks * 64
    o_lw = o_part + n_tiles * 64
    o_parts = o_lw + M * 64
    o_tab = o_parts + M * 128
    o_flag = o_tab + M + 1
    need = o_flag + (tasks + 1) // 2
    want = [("z", 0), ("eps", o_eps), ("beta", o_beta), ("c", o_c), ("part", o_part), ("lw", o_lw), ("parts", o_parts),
            ("tab", o_tab), ("flag", o_flag), ("need", need)]
    sizes = {"z": rows * L, **_sample_sizes(M, L, R, tasks, n_tiles, 64), "flag": (tasks + 1) // 2}
    _check(_run(driver, "marginal", rows, L, R, M, n_tiles), want, sizes)


@pytest.mark.parametrize("K", [0, 1, 130])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_joint_layout(driver, shape, K):
    _, L, R, N, M, rows, tasks, n_tiles, n_blk = _dims(shape)
    work = 1000 + 7 * rows  # (joint_work_doubles: any count)
    o_stats = work
    o_v = o_stats + 8 * M
    o_eps = o_v + rows * L
    o_beta = o_eps + (tasks * R * 64 if K else 0)
    o_c = o_beta + (tasks * R * 64 if K else 0)
    o_part = o_c + (tasks * 64 if K else 0)
    o_lw = o_part + (n_tiles * 64 if K else 0)
    o_parts = o_lw + (M * 64 if K else 0)
    o_tab = o_parts + (M * 128 if K else 0)
    need = o_tab + M + 1
    want = [("work", 0), ("stats", o_stats), ("v", o_v), ("eps", o_eps), ("beta", o_beta), ("c", o_c), ("part", o_part),
            ("lw", o_lw), ("parts", o_parts), ("tab", o_tab), ("need", need)]
    sizes = {"work": work, "stats": 8 * M, "v": rows * L, **_sample_sizes(M, L, R, tasks, n_tiles, 64 if K else 0)}
    if not K:
        assert o_eps == o_tab  # the optional regions collapse
    _check(_run(driver, "joint", work, rows, L, R, M, n_tiles, K), want, sizes)
