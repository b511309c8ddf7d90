"""The gather that fills a pair batch's target pool from a cross batch's pack of many targets
(edlib_amd/csrc/pairs_gather_core.hpp: cell_base, target_run_cells; edlibAmdBatchPairsSetCells) without a GPU: the DEVICE
code compiled for the host (tests/pairs_gather_cells_host.cpp: the same header, the plan and the destination runs walked
one by one in the kernels' order) against plain numpy slicing -- targets of the lengths around the dword and run sizes
packed dword-aligned in (length, index) order, every nibble phase of a window's start with every window length, windows
that end on a target's last base with the next target's codes directly behind, the last target of the pack up to its last
base, pairs shorter than a run so that a run spans three and more pairs, a pool whose size is no multiple of 16, targets
of 1 to 16 symbols, and a window whose nibble position lies above 2^31.  The same source with its own main() runs under
the address and undefined-behaviour sanitizers as a child process.  The query pool's gather is the one of
tests/test_pairs_gather_model.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pairs_set_cases import WINDOW_LENGTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pairs_gather_cells_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "pairs_gather_core.hpp")

# the caller's order, lengths repeated; 407: a window of 400 bases at every phase
TARGET_LENGTHS = (33, 1, 400, 8, 2, 17, 7, 64, 407, 9, 16, 15, 32, 31, 8, 400, 407)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libpairs_gather_cells_host.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.pairs_gather_cells_host.restype = ctypes.c_int
    lib.pairs_gather_cells_host.argtypes = [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + \
                                           [ctypes.c_void_p] * 5
    return lib


def _alphabet(rng, sigma):
    """`sigma` distinct bytes in ascending order; with more than one the top code is a byte >= 128"""
    a = np.array(sorted(rng.choice(np.arange(33, 200), size=sigma, replace=False)), dtype=np.uint8)
    if sigma > 1:
        a[-1] = 200 + sigma
    return a


def _targets(rng, alphabet, lengths):
    out = []
    for n in lengths:
        t = alphabet[rng.integers(0, len(alphabet), n)]
        t[::7] = alphabet[-1]                                            # the top code is in use
        out.append(t)
    return out


def _pack(targets, alphabet, first_dword=0):
    """a cross batch's pack: the targets in (length, index) order, each from a dword of its own, 4 bits a column, LSB
    first; returns the dwords from first_dword on, place (target -> place in the order) and tdw (place -> first dword)"""
    order = sorted(range(len(targets)), key=lambda t: (len(targets[t]), t))
    place = np.zeros(len(targets), dtype=np.int32)
    tdw = np.zeros(len(targets), dtype=np.int64)
    words = []
    at = first_dword
    for i, t in enumerate(order):
        place[t], tdw[i] = i, at
        codes = np.searchsorted(alphabet, targets[t]).astype(np.uint32)
        padded = np.zeros((len(codes) + 7) // 8 * 8, dtype=np.uint32)
        padded[:len(codes)] = codes
        words.append((padded.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1).astype(np.uint32))
        at += len(words[-1])
    table = np.zeros(16, dtype=np.uint8)
    table[:len(alphabet)] = alphabet
    return np.concatenate(words), place, tdw, table


def _gather(host, pack, ndw, table, place, tdw, pt, ps, pl):
    pt, pl = (np.ascontiguousarray(a, dtype=np.int32) for a in (pt, pl))
    ps = None if ps is None else np.ascontiguousarray(ps, dtype=np.int32)
    n = len(pt)
    toff = np.zeros(n + 1, dtype=np.int64)
    toff[1:] = np.cumsum(pl)
    base = np.zeros(n, dtype=np.int64)
    tout = np.full(toff[n] + 16 + 64, 0xEE, dtype=np.uint8)               # (64 guard bytes behind the pool)
    assert host.pairs_gather_cells_host(pack.ctypes.data, ndw, table.ctypes.data, place.ctypes.data, tdw.ctypes.data, n,
                                        toff.ctypes.data, pt.ctypes.data, None if ps is None else ps.ctypes.data,
                                        base.ctypes.data, tout.ctypes.data) == 0
    return tout, toff, base


def _check(host, targets, alphabet, pt, ps, pl):
    pack, place, tdw, table = _pack(targets, alphabet)
    tout, toff, base = _gather(host, pack, len(pack), table, place, tdw, pt, ps, pl)
    starts = [0] * len(pt) if ps is None else ps
    want = np.concatenate([targets[t][s:s + n] for t, s, n in zip(pt, starts, pl)] + [np.zeros(16, dtype=np.uint8)])
    assert np.array_equal(base, 8 * tdw[place[np.asarray(pt)]] + np.asarray(starts))
    assert np.array_equal(tout[:len(want)], want), np.flatnonzero(tout[:len(want)] != want)[:8]
    assert (tout[len(want):] == 0xEE).all()                               # nothing behind the pool
    return len(want) - 16


def grid(rng, targets):
    """every nibble phase of the start x every window length (in the 407-base targets), windows that end on every
    target's last base, every target whole, runs of one- and two-byte pairs"""
    pt, ps, pl = [], [], []
    long_ones = [t for t in range(len(targets)) if len(targets[t]) >= 407]
    for phase in range(8):
        for n in WINDOW_LENGTHS:
            t = long_ones[(phase + n) % len(long_ones)]
            s = phase + 8 * int(rng.integers(0, (len(targets[t]) - n - phase) // 8 + 1))
            pt.append(t); ps.append(s); pl.append(n)
    for t in range(len(targets)):
        L = len(targets[t])
        pt += [t, t]; ps += [0, L - 1]; pl += [L, 1]
        for n in WINDOW_LENGTHS:
            if n < L:
                pt.append(t); ps.append(L - n); pl.append(n)              # ends on the target's last base
    for i in range(40):                                                   # pairs of 1 and 2 bytes in a row
        t = i % len(targets)
        L = len(targets[t])
        n = min(1 + (i & 1), L)
        pt.append(t); ps.append(int(rng.integers(0, L - n + 1))); pl.append(n)
    return pt, ps, pl


@pytest.mark.parametrize("sigma", [1, 4, 5, 16])
def test_grid_against_numpy_slicing(host, sigma):
    rng = np.random.default_rng(200 + sigma)
    alphabet = _alphabet(rng, sigma)
    targets = _targets(rng, alphabet, TARGET_LENGTHS)
    if sigma == 16:
        assert all(t.max() >= 128 for t in targets) and alphabet[15] >= 128
    pt, ps, pl = grid(rng, targets)
    # every phase x every length is there
    seen = {(s % 8, n) for s, n in zip(ps, pl)}
    assert all((phase, n) in seen for phase in range(8) for n in WINDOW_LENGTHS)
    # the last target of the pack up to its last base
    last = max(range(len(targets)), key=lambda t: (len(targets[t]), t))
    assert any(t == last and s + n == len(targets[last]) for t, s, n in zip(pt, ps, pl))
    total = _check(host, targets, alphabet, pt, ps, pl)
    if total % 16 == 0:
        pt.append(0); ps.append(0); pl.append(1)
        total = _check(host, targets, alphabet, pt, ps, pl)
    assert total % 16 != 0
    order = rng.permutation(len(pt))                                      # another alignment of every boundary
    _check(host, targets, alphabet, *[[a[i] for i in order] for a in (pt, ps, pl)])
    # the whole-target form: no starts
    whole = list(rng.permutation(len(targets))) * 2
    _check(host, targets, alphabet, whole, None, [len(targets[t]) for t in whole])


def test_many_blocks_and_short_pairs(host):
    """more than one block of 4,096 bytes, and 600 pairs of one to three bytes: every run spans five pairs and more"""
    rng = np.random.default_rng(9)
    alphabet = _alphabet(rng, 5)
    targets = _targets(rng, alphabet, list(rng.integers(1, 700, 80)) + [65536, 1, 1])
    pt = list(rng.integers(0, len(targets), 900))
    pl = [int(rng.integers(1, min(len(targets[t]), 3 if i < 600 else 500) + 1)) for i, t in enumerate(pt)]
    ps = [int(rng.integers(0, len(targets[t]) - n + 1)) for t, n in zip(pt, pl)]
    pt.append(80); ps.append(0); pl.append(65536)
    assert _check(host, targets, alphabet, pt, ps, pl) > 3 * 4096


def test_a_base_above_two_to_the_31_nibbles(host):
    """a pack of a little over 1 GiB whose last few KiB alone are written and read: the windows start above nibble 2^31"""
    first = (1 << 28) + 3                                                 # the first dword that holds a target
    rng = np.random.default_rng(31)
    alphabet = _alphabet(rng, 16)
    targets = _targets(rng, alphabet, TARGET_LENGTHS)
    tail, place, tdw, table = _pack(targets, alphabet, first_dword=first)
    try:
        pack = np.zeros(first + len(tail), dtype=np.uint32)              # (zero pages: nothing is touched below `first`)
    except MemoryError:
        pytest.skip("no memory for a zero-filled array of 1 GiB")
    pack[first:] = tail
    pt, ps, pl = grid(rng, targets)
    tout, toff, base = _gather(host, pack, len(pack), table, place, tdw, pt, ps, pl)
    assert base.min() > 2 ** 31
    want = np.concatenate([targets[t][s:s + n] for t, s, n in zip(pt, ps, pl)] + [np.zeros(16, dtype=np.uint8)])
    assert np.array_equal(tout[:len(want)], want), np.flatnonzero(tout[:len(want)] != want)[:8]
    assert (tout[len(want):] == 0xEE).all()
    del pack


def test_sanitizer_build_runs_clean():
    """the same source with its own main(), -fsanitize=address,undefined, as a child process"""
    exe = os.path.join(ROOT, "build", "pairs_gather_cells_host_san")
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
        r = subprocess.run(["g++"] + flags + ["-DPAIRS_GATHER_MAIN", "-o", exe, SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout, r.stdout
