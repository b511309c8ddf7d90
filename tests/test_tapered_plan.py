"""The tapered segmentation of the last level's main launch (edlib_amd/csrc/segment_plan.hpp) without a GPU: the
header compiled for the host (tests/tapered_plan_host.cpp).  The table covers [0, T) exactly, in ascending order, on starts
that are multiples of 16; the lengths never grow and stay within [four warm-ups, the uniform length] except for the ragged
last one; there are at most 65,535 segments; and where a taper cannot pay (the uniform length is no more than four warm-ups,
or the launch is under two rounds of resident workgroups) the table is the uniform plan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESIDENT = 2048          # 8 workgroups of 4 waves on each of 256 CUs
WARM = 319               # 2 x 160 - 1: the warm-up of a group of five words (150-base reads)


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libtapered_plan_host.so")
    src = os.path.join(ROOT, "tests", "tapered_plan_host.cpp")
    hdr = os.path.join(ROOT, "edlib_amd", "csrc", "segment_plan.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.plan_uniform_host.restype = None
    lib.plan_uniform_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
    lib.plan_tapered_host.restype = ctypes.c_int
    lib.plan_tapered_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def uniform(lib, rblocks, T, warm=WARM):
    """(S, segLen, warm) of the launch's uniform plan (the engine's call: 65,536 waves wanted, segments >= 4,096 columns)"""
    out = (ctypes.c_int * 3)()
    lib.plan_uniform_host(rblocks * 64, T, warm, 65536, 4096, out)
    return out[0], out[1], out[2]


def tapered(lib, T, grid_x, resident, warm, lmax):
    room = 70000
    out = (ctypes.c_int * (2 * room))()
    n = lib.plan_tapered_host(T, grid_x, resident, warm, lmax, out, room)
    assert 0 < n <= room
    return np.array(out[:2 * n], dtype=np.int64).reshape(n, 2)


def uniform_table(T, lmax):
    starts = np.arange(0, T, lmax, dtype=np.int64)
    return np.stack([starts, np.minimum(lmax, T - starts)], axis=1)


def check_table(t, T, warm, lmax):
    min_cols = max(16, (4 * warm + 15) // 16 * 16)
    start, cols = t[:, 0], t[:, 1]
    assert start[0] == 0 and np.all(cols > 0)
    assert np.array_equal(start[1:], start[:-1] + cols[:-1])            # ascending, no gap, no overlap
    assert start[-1] + cols[-1] == T                                      # exact cover
    assert np.all(start % 16 == 0)
    assert np.all(np.diff(cols) <= 0)                                     # never longer than the one before
    assert np.all(cols[:-1] % 16 == 0)
    assert np.all(cols[:-1] >= min_cols) and np.all(cols <= lmax)
    assert len(t) <= 65535


@pytest.mark.parametrize("T,rblocks", [(5_000_000, 788), (2_000_000, 256), (4_999_999, 788), (5_000_001, 788),
                                       (1_999_999, 256), (2_000_001, 256)])
def test_taper(host, T, rblocks):
    S, lmax, warm = uniform(host, rblocks, T)
    grid_x = (rblocks + 3) // 4
    assert warm == WARM and grid_x * S >= 2 * RESIDENT
    t = tapered(host, T, grid_x, RESIDENT, warm, lmax)
    check_table(t, T, warm, lmax)
    cols = t[:, 1]
    # a real taper: it starts at the uniform length, goes down to four warm-ups, and every length in between is the share
    # remaining / (2 R) of what was left when it was cut
    assert cols[0] == lmax and 1280 in cols[:-1] and len(t) > S
    rem = T - t[:, 0]
    want = np.clip(rem * grid_x // (2 * RESIDENT) // 16 * 16, 1280, lmax)
    assert np.array_equal(cols[:-1], want[:-1]) and cols[-1] == min(want[-1], rem[-1])
    print("T=%d: %d uniform segments of %d -> %d tapered, %d at the uniform length, %d at 1,280, warm-up columns %d -> %d"
          % (T, S, lmax, len(t), int(np.sum(cols == lmax)), int(np.sum(cols == 1280)), (S - 1) * warm, (len(t) - 1) * warm))


def test_headline_shape(host):
    """1M reads leave ~50,400: 197 workgroups per segment, 84 uniform segments of 59,536 columns"""
    S, lmax, warm = uniform(host, 788, 5_000_000)
    assert (S, lmax) == (84, 59536)
    t = tapered(host, 5_000_000, 197, RESIDENT, warm, lmax)
    assert 140 <= len(t) <= 170
    assert (len(t) - S) * warm < 0.006 * 5_000_000                        # the warm-ups added: under 0.6 % of the columns


@pytest.mark.parametrize("T,rblocks", [(65_536, 788), (65_536, 256), (4_799, 788), (4_799, 256), (2_000_000, 16)])
def test_under_two_rounds_is_uniform(host, T, rblocks):
    S, lmax, warm = uniform(host, rblocks, T)
    grid_x = (rblocks + 3) // 4
    assert grid_x * S < 2 * RESIDENT
    t = tapered(host, T, grid_x, RESIDENT, warm, lmax)
    assert len(t) == S and np.array_equal(t, uniform_table(T, lmax))
    check_table(t, T, 0, lmax)


@pytest.mark.parametrize("lmax", [1280, 1264, 608])
def test_uniform_length_within_four_warmups_is_uniform(host, lmax):
    T = 5_000_000
    t = tapered(host, T, 197, RESIDENT, WARM, lmax)
    assert np.array_equal(t, uniform_table(T, lmax))


def test_segment_limit(host):
    """a target near 2^31 columns with no warm-up: the shortest segment grows until 65,535 are enough"""
    T = 2**31 - 17
    t = tapered(host, T, 197, RESIDENT, 0, 32800)
    check_table(t, T, 0, 32800)
    assert 60000 < len(t) <= 65535
