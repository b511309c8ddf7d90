"""The batch of tests/test_gpu_tapered_segments.py, shared with its child process (tests/tapered_child.py): 16,384 reads of 150
bases against 2,000,003 columns (not a multiple of 16), all of them above every threshold but the full one, so that the last
level's main launch scans them all on tapered segments (256 read blocks; edlib_amd/csrc/segment_plan.hpp through
tests/tapered_plan_host.cpp gives the table).  Most reads are unrelated sequence (best distance 54 .. 66); the planted ones sit
SUBS substitutions from the target, where the segments meet."""
import ctypes
import os
import subprocess

import numpy as np

from edlib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 2_000_003
N = 16_384
M = 150
SUBS = 40                # above 32 (a ladder level this batch could take would be at most that), below what random sequence reaches
RESIDENT = 2048          # workgroups of the scan resident on 256 CUs (the library's debug line confirms the segment count)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def plan_lib():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libtapered_plan_host.so")
    src = os.path.join(ROOT, "tests", "tapered_plan_host.cpp")
    hdr = os.path.join(ROOT, "edlib_amd", "csrc", "segment_plan.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def table():
    """(start, columns) of the main launch's segments for this batch, and the uniform length"""
    lib = plan_lib()
    u = (ctypes.c_int * 3)()
    lib.plan_uniform_host(N, T, 2 * 32 * ((M + 31) // 32) - 1, ctypes.c_longlong(65536), 4096, u)
    room = 4096
    out = (ctypes.c_int * (2 * room))()
    n = lib.plan_tapered_host(T, (N // 64 + 3) // 4, RESIDENT, u[2], u[1], out, room)
    assert 0 < n <= room
    return np.array(out[:2 * n], dtype=np.int64).reshape(n, 2), u[1]


def _mutate(rng, block):
    """SUBS substitutions, none in the first or the last five bases (an edit at an end ties with the neighbouring column)"""
    r = np.array(block, dtype=np.uint8)
    at = rng.choice(np.arange(5, M - 5), SUBS, replace=False)
    for i in at:
        r[i] = rng.choice(_ACGT[_ACGT != r[i]])
    return r


def batch():
    """{"reads", "target", "planted": {name: read index}, "ends": {name: the end columns the read was planted at}, "table"}"""
    tab, lmax = table()
    start, cols = tab[:, 0], tab[:, 1]
    n = len(tab)
    rng = np.random.default_rng(1409)
    target = synth.random_dna(1401, T).copy()
    i_long = 10
    i_short = int(np.argmax(cols == 1280)) + 3
    assert cols[i_long] == lmax and cols[i_long + 4] == lmax and cols[n - 2] == 1280 and i_short + 20 < n - 2
    planted, ends = {}, {}

    def copy_block(src, dst):
        target[dst:dst + M] = target[src:src + M]

    def tandem(at, repeats):
        unit = _ACGT[rng.integers(0, 4, 10)]
        while len(set(unit.tolist())) < 4 or np.array_equal(unit[:5], unit[5:]):
            unit = _ACGT[rng.integers(0, 4, 10)]
        target[at:at + M + 10 * (repeats - 1)] = np.tile(unit, 15 + repeats - 1)
        return np.tile(unit, 15)

    # (1) the target first: two copied blocks and two tandem regions
    a1, b1 = int(start[i_long + 3]) + 1000, int(start[i_short + 5]) + 300          # one end in a long, one in a short segment
    copy_block(a1, b1)
    a2, b2 = int(start[i_short + 8]) + 200, int(start[i_short + 9]) + 200          # two short segments
    copy_block(a2, b2)
    t1 = int(start[i_short + 12]) + 100                                            # 20 ends inside one short segment
    rep1 = tandem(t1, 20)
    t2 = int(start[i_short + 15]) - (M - 1) - 100                                  # 10 ends before a boundary, 10 after
    rep2 = tandem(t2, 20)
    # (2) the reads
    case = {}

    def at_end(name, e):                                                           # a read ending on column e
        case[name] = _mutate(rng, target[e - M + 1:e + 1]); ends[name] = [e]

    at_end("tail", int(start[n - 2]) + 600)
    at_end("long_last", int(start[i_long + 1]) - 1)
    at_end("long_first", int(start[i_long + 1]))
    at_end("short_last", int(start[i_short + 1]) - 1)
    at_end("short_first", int(start[i_short + 1]))
    at_end("target_end", T - 1)
    case["two_long_short"] = _mutate(rng, target[a1:a1 + M]); ends["two_long_short"] = [a1 + M - 1, b1 + M - 1]
    case["two_short_short"] = _mutate(rng, target[a2:a2 + M]); ends["two_short_short"] = [a2 + M - 1, b2 + M - 1]
    case["many_in_one"] = _mutate(rng, rep1); ends["many_in_one"] = [t1 + M - 1 + 10 * j for j in range(20)]
    case["many_across"] = _mutate(rng, rep2); ends["many_across"] = [t2 + M - 1 + 10 * j for j in range(20)]
    reads = [np.ascontiguousarray(x) for x in _ACGT[rng.integers(0, 4, (N, M))]]
    for j, name in enumerate(sorted(case)):
        planted[name] = 37 + 1500 * j                                              # scattered over the waves
        reads[planted[name]] = np.ascontiguousarray(case[name])
    return {"reads": reads, "target": target, "planted": planted, "ends": ends, "table": tab}
