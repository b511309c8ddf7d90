"""The gather that fills a pair batch's target pool from a read batch's raw target (edlib_amd/csrc/pairs_gather_core.hpp:
bytes16, target_run_bytes; edlibAmdBatchPairsSetSharedWindows) without a GPU: the DEVICE code compiled for the host
(tests/pairs_gather_bytes_host.cpp: the same header, the destination runs walked one by one in the kernel's order) against
plain numpy slicing -- a target of 1,031 bytes over 40 byte values, every source byte phase against every destination
phase for window lengths around the run and dword sizes, windows at column 0 and ending at the last column, and the 16
zero bytes behind the pool.  The same source with its own main() runs under the address and undefined-behaviour
sanitizers as a child process.  The query pool's gather is the one of tests/test_pairs_gather_model.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pairs_gather_bytes_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "pairs_gather_core.hpp")

WINDOW_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400)
T = 1031


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libpairs_gather_bytes_host.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.pairs_gather_bytes_host.restype = ctypes.c_int
    lib.pairs_gather_bytes_host.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.pairs_gather_bytes16.restype = None
    lib.pairs_gather_bytes16.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def target():
    """1,031 bytes over 40 distinct values, some >= 128"""
    rng = np.random.default_rng(1031)
    alphabet = np.concatenate([6 * np.arange(39) + 7, [255]]).astype(np.uint8)
    t = alphabet[rng.integers(0, 40, T)]
    t[::41] = alphabet[np.arange(len(t[::41])) % 40]
    assert len(np.unique(t)) == 40 and (t >= 128).any()
    return t


def _words(target):
    """what the kernel may read: the whole dwords of a read batch's target pool, the target and 16 bytes behind it"""
    raw = np.concatenate([target, np.zeros(16, dtype=np.uint8)])
    words = np.zeros(len(raw) // 4, dtype=np.uint32)
    words.view(np.uint8)[:] = raw[:4 * len(words)]
    return words


def _check(host, target, ps, pl):
    words = _words(target)
    ps, pl = (np.ascontiguousarray(a, dtype=np.int32) for a in (ps, pl))
    assert (ps >= 0).all() and (pl >= 1).all() and (ps + pl <= len(target)).all()
    n = len(ps)
    toff = np.zeros(n + 1, dtype=np.int64)
    toff[1:] = np.cumsum(pl)
    tout = np.full(toff[n] + 16 + 64, 0xEE, dtype=np.uint8)              # (64 guard bytes behind the pool)
    assert host.pairs_gather_bytes_host(words.ctypes.data, len(words), n, toff.ctypes.data, ps.ctypes.data,
                                        tout.ctypes.data) == 0
    want = np.concatenate([target[s:s + n] for s, n in zip(ps, pl)] + [np.zeros(16, dtype=np.uint8)])
    assert np.array_equal(tout[:len(want)], want), np.flatnonzero(tout[:len(want)] != want)[:8]
    assert (tout[len(want):] == 0xEE).all()                                # nothing behind the pool
    return toff


def phase_grid(rng, target_length):
    """every window length x every source byte phase 0..3 x every destination phase 0..15 (a filler pair in front moves
    the pool to it), then windows at column 0 and ending at the last column, and the whole target"""
    ps, pl, seen = [], [], set()
    total = 0
    for n in WINDOW_LENGTHS:
        for sp in range(4):
            for dp in range(16):
                fill = (dp - total) % 16
                if fill:
                    ps.append(int(rng.integers(0, target_length - 16)))
                    pl.append(fill)
                    total += fill
                s = 4 * int(rng.integers(0, (target_length - n - sp) // 4 + 1)) + sp
                seen.add((n, s % 4, total % 16))
                ps.append(s)
                pl.append(n)
                total += n
    assert len(seen) == len(WINDOW_LENGTHS) * 4 * 16
    for n in WINDOW_LENGTHS:
        ps += [0, target_length - n]
        pl += [n, n]
    ps.append(0)
    pl.append(target_length)
    return ps, pl


def test_bytes16_at_every_position(host, target):
    """five dwords funnel-shifted: every byte phase, and zero behind the last dword of the block"""
    words = _words(target)
    raw = np.concatenate([words.view(np.uint8), np.zeros(32, dtype=np.uint8)])
    out = np.zeros(16, dtype=np.uint8)
    for s in range(4 * len(words) + 8):
        host.pairs_gather_bytes16(words.ctypes.data, len(words), s, out.ctypes.data)
        assert np.array_equal(out, raw[s:s + 16]), s


def test_phase_grid_against_numpy_slicing(host, target):
    rng = np.random.default_rng(5)
    ps, pl = phase_grid(rng, len(target))
    _check(host, target, ps, pl)
    order = rng.permutation(len(ps))                                       # the same pairs, every boundary elsewhere
    _check(host, target, [ps[i] for i in order], [pl[i] for i in order])


def test_one_pair_many_blocks_and_one_byte_pairs(host, target):
    rng = np.random.default_rng(6)
    for n in WINDOW_LENGTHS:
        for s in (0, 1, 2, 3, len(target) - n):
            _check(host, target, [s], [n])
    # more than one block of 4,096 destination bytes, one-byte pairs in a row, a window of 65,536 columns of a long target
    pl = list(rng.integers(1, 420, 300)) + [1] * 50
    ps = [int(rng.integers(0, len(target) - n + 1)) for n in pl]
    _check(host, target, ps, pl)
    long_target = np.random.default_rng(8).integers(0, 256, 70001).astype(np.uint8)
    _check(host, long_target, [5, 4465, 70001 - 33, 3], [17, 65536, 33, 65536])


def test_sanitizer_build_runs_clean():
    """the same source with its own main(), -fsanitize=address,undefined, as a child process"""
    exe = os.path.join(ROOT, "build", "pairs_gather_bytes_host_san")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (the runtimes linked into the program: it runs whatever else the loader brings in front of it)
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan", "-static-libubsan"]
    if _stale(exe):
        # does the toolchain link these runtimes at all?  A trivial program says; the real source must then build
        probe = os.path.join(ROOT, "build", "sanitizer_probe")
        r = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("the compiler here does not link the sanitizer runtimes: " + r.stderr.strip()[-200:])
        r = subprocess.run(["g++"] + flags + ["-DPAIRS_GATHER_BYTES_MAIN", "-o", exe, SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout, r.stdout
