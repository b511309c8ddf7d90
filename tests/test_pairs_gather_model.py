"""The gather that fills a pair batch's pools from a window batch (edlib_amd/csrc/pairs_gather_core.hpp) without a GPU: the
DEVICE code compiled for the host (tests/pairs_gather_host.cpp: the same header, the destination runs walked one by one in
the kernel's order) against plain numpy slicing -- the nibble phase of a window's first column, window lengths around the
run and dword sizes, every alignment of a pair boundary inside a 16-byte run, the target's two ends, targets of 1 to 16
symbols, queries on both strands from a plain and from a stranded pool, and the 16 zero bytes behind both pools.  The same
source with its own main() runs under the address and undefined-behaviour sanitizers as a child process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edlib_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pairs_gather_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "pairs_gather_core.hpp")

WINDOW_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400)
QUERY_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256)
QUERY_BYTES = np.frombuffer(b"ACGTNacgtnUuRYKMBVDHSWrykmbvdhsw-*", dtype=np.uint8)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libpairs_gather_host.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.pairs_gather_host.restype = ctypes.c_int
    lib.pairs_gather_host.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def comp():
    """the 256 complements, from edlibAmdReverseComplement itself"""
    return np.array([edlib_amd.reverse_complement(bytes([b]))[0] for b in range(256)], dtype=np.uint8)


def _pack(target):
    """a window batch's pack: ids in ascending byte order, 4 bits a column, 8 columns a dword, LSB first"""
    ids = np.unique(target)
    assert len(ids) <= 16
    codes = np.searchsorted(ids, target).astype(np.uint32)
    padded = np.zeros((len(target) + 7) // 8 * 8, dtype=np.uint32)
    padded[:len(target)] = codes
    pack = (padded.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    table = np.zeros(16, dtype=np.uint8)
    table[:len(ids)] = ids
    return pack, table


def _pool(queries, stranded):
    """a window batch's query pool: entry q, or 2 q (the query) and 2 q + 1 (its reverse complement) where stranded"""
    entries = []
    for q in queries:
        entries.append(q)
        if stranded:
            entries.append(edlib_amd.reverse_complement(q))
    off = np.zeros(len(entries) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in entries])
    raw = np.concatenate(entries + [np.zeros(16, dtype=np.uint8)])
    words = np.zeros(len(raw) // 4, dtype=np.uint32)                   # what the kernel may read: whole dwords of the block
    words.view(np.uint8)[:] = raw[:4 * len(words)]
    return words, off


def _check(host, comp, target, queries, stranded, pq, ps, pl, pst):
    qout, tout, qoff, toff = _gather_call(host, comp, target, queries, stranded, pq, ps, pl, pst)
    want_t = np.concatenate([target[s:s + n] for s, n in zip(ps, pl)] + [np.zeros(16, dtype=np.uint8)])
    want_q = np.concatenate([(edlib_amd.reverse_complement(queries[q]) if (pst is not None and pst[i]) else queries[q])
                             for i, q in enumerate(pq)] + [np.zeros(16, dtype=np.uint8)])
    assert np.array_equal(tout[:len(want_t)], want_t), np.flatnonzero(tout[:len(want_t)] != want_t)[:8]
    assert np.array_equal(qout[:len(want_q)], want_q), np.flatnonzero(qout[:len(want_q)] != want_q)[:8]
    assert (tout[len(want_t):] == 0xEE).all() and (qout[len(want_q):] == 0xEE).all()      # nothing behind the pools


def _gather_call(host, comp, target, queries, stranded, pq, ps, pl, pst):
    pack, table = _pack(target)
    words, srcoff = _pool(queries, stranded)
    pq, ps, pl = (np.ascontiguousarray(a, dtype=np.int32) for a in (pq, ps, pl))
    pst = None if pst is None else np.ascontiguousarray(pst, dtype=np.uint8)
    n = len(pq)
    qoff = np.zeros(n + 1, dtype=np.int64)
    toff = np.zeros(n + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(queries[q]) for q in pq])
    toff[1:] = np.cumsum(pl)
    qout = np.full(qoff[n] + 16 + 64, 0xEE, dtype=np.uint8)             # (64 guard bytes behind each pool)
    tout = np.full(toff[n] + 16 + 64, 0xEE, dtype=np.uint8)
    assert host.pairs_gather_host(pack.ctypes.data, len(pack), table.ctypes.data, words.ctypes.data, len(words),
                                  srcoff.ctypes.data, int(stranded), comp.ctypes.data, n, qoff.ctypes.data,
                                  toff.ctypes.data, pq.ctypes.data, ps.ctypes.data,
                                  None if pst is None else pst.ctypes.data, qout.ctypes.data, tout.ctypes.data) == 0
    return qout, tout, qoff, toff


def _target(rng, sigma, length):
    """`sigma` distinct bytes, some of them >= 128; with 16 of them the highest code (15) is used"""
    alphabet = np.array(sorted(rng.choice(np.arange(33, 256), size=sigma, replace=False)), dtype=np.uint8)
    if sigma > 1:
        alphabet[-1] = 200 + sigma                                       # (a byte >= 128 among them, and it is the top code)
    t = alphabet[rng.integers(0, sigma, length)]
    t[::7] = alphabet[-1]
    return t


def _queries(rng):
    return [QUERY_BYTES[rng.integers(0, len(QUERY_BYTES), m)] for m in QUERY_LENGTHS]


def grid(rng, target_length, num_queries):
    """every nibble phase x every window length, and runs of consecutive odd lengths that put the next pair's first byte
    at every alignment; windows at column 0 and ending at the target's last column; both strands"""
    pq, ps, pl = [], [], []
    for phase in range(8):
        for n in WINDOW_LENGTHS:
            ps.append(8 * int(rng.integers(0, (target_length - 400) // 8 - 1)) + phase)
            pl.append(n)
    for n in (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33):
        ps.append(int(rng.integers(0, target_length - 40)))
        pl.append(n)
    for n in WINDOW_LENGTHS:
        ps.append(0); pl.append(n)
        ps.append(target_length - n); pl.append(n)
    ps.append(0); pl.append(target_length)
    pq = [i % num_queries for i in range(len(ps))]
    pst = [(i // num_queries) & 1 for i in range(len(ps))]
    return pq, ps, pl, pst


@pytest.mark.parametrize("sigma", [1, 4, 5, 16])
@pytest.mark.parametrize("stranded", [False, True])
def test_grid_against_numpy_slicing(host, comp, sigma, stranded):
    rng = np.random.default_rng(100 + sigma)
    target = _target(rng, sigma, 5003)
    if sigma == 16:
        assert len(np.unique(target)) == 16 and target.max() >= 128
    queries = _queries(rng)
    pq, ps, pl, pst = grid(rng, len(target), len(queries))
    _check(host, comp, target, queries, stranded, pq, ps, pl, pst)
    _check(host, comp, target, queries, stranded, pq, ps, pl, None)                 # all forward
    order = rng.permutation(len(pq))                                                 # another alignment of every boundary
    _check(host, comp, target, queries, stranded, *[[a[i] for i in order] for a in (pq, ps, pl, pst)])


def test_one_pair_and_many_blocks(host, comp):
    rng = np.random.default_rng(7)
    target = _target(rng, 4, 70001)
    queries = _queries(rng)
    for m in range(len(queries)):
        for strand in (0, 1):
            _check(host, comp, target, queries, False, [m], [int(rng.integers(0, 1000))], [1 + m], [strand])
    # more than one block of 4,096 bytes per pool, a window of 65,536 columns, one-byte pairs in a row
    pq = list(rng.integers(0, len(queries), 300)) + [0] * 50
    pl = list(rng.integers(1, 420, 300)) + [1] * 50
    ps = [int(rng.integers(0, len(target) - n)) for n in pl]
    pst = list(rng.integers(0, 2, 350))
    pq.append(8); ps.append(4465); pl.append(65536); pst.append(1)
    for stranded in (False, True):
        _check(host, comp, target, queries, stranded, pq, ps, pl, pst)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 300000])
def test_both_searches_find_the_pair_of_a_byte(host, n):
    """the thread's binary search and the wave's search by 64 probes a step against numpy's searchsorted: pairs of one
    byte and of many, every position around a pair's first byte, both ends of the pool"""
    rng = np.random.default_rng(n)
    host.pairs_gather_host_find.restype = ctypes.c_int
    host.pairs_gather_host_find.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    for longest in (1, 2, 400):
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum(rng.integers(1, longest + 1, size=n))
        at = rng.integers(0, n, size=60)
        positions = np.unique(np.clip(np.concatenate([off[at], off[at] - 1, off[at] + 1, [0, off[n] - 1]]), 0, off[n] - 1))
        want = np.searchsorted(off, positions, side="right") - 1
        for pos, p in zip(positions, want):
            for wave in (0, 1):
                assert host.pairs_gather_host_find(off.ctypes.data, 0, n - 1, int(pos), wave) == p, (n, longest, pos, wave)
            # a range that starts at a pair below, as the block's second search does
            lo = max(int(p) - 3, 0)
            assert host.pairs_gather_host_find(off.ctypes.data, lo, min(lo + 4096, n - 1), int(pos), 1) == p


def test_sanitizer_build_runs_clean():
    """the same source with its own main(), -fsanitize=address,undefined, as a child process"""
    exe = os.path.join(ROOT, "build", "pairs_gather_host_san")
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
