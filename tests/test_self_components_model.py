"""The components of a self batch (edlibAmdBatchSelfComponents) without a GPU.
  * self_components_model() -- the statement the GPU tests compare with -- against scipy's connected_components where
    scipy imports, else against a dense transitive closure (n <= 60); the canonical-label and member-order rules are
    checked on their own.
  * The DEVICE code of the union-find (edlib_amd/csrc/self_components_core.hpp) compiled for the host
    (tests/self_components_host.cpp: __atomic builtins in place of the agent-scope atomics): chains, stars, cliques,
    forests and duplicated edges over n = 1 .. 300, every edge list in several shuffled orders and from 1, 2 and 8
    threads that split the edges, equal every time to the serial minimum-label answer; the hit-list and the dense form
    with pairs above the level and unreported pairs between the edges.
  * The same source with its own main() as a program of its own under the address + undefined-behaviour sanitizers and,
    a second build, under the thread sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "self_components_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "self_components_core.hpp")


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libself_components_host.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.self_components_host_edges.argtypes = [I, P, P, LL, I, P]
    lib.self_components_host_hits.argtypes = [I, P, P, P, LL, I, P, I, P]
    lib.self_components_host_dense.argtypes = [I, P, I, I, P]
    return lib


def serial_labels(n, ei, ej):
    """the ten-line union-find: union by minimum, the label is the smallest index of the component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in zip(ei, ej):
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def graph(rng, n, shape):
    """edges of one of the shapes over a random naming of the vertices, with every third edge again, turned round"""
    name = rng.permutation(n)
    e = []
    if shape == "chain":
        e = [(i, i + 1) for i in range(n - 1)]
    elif shape == "star":
        e = [(n - 1, i) for i in range(n - 1)]
    elif shape == "cliques":
        e = [(i, j) for i in range(n) for j in range(i + 1, n) if i // 9 == j // 9]
    elif shape == "forest":
        e = [(i, int(rng.integers(0, i))) for i in range(1, n) if i % 11]
    elif shape == "sparse":
        e = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(n, 2)) if a != b]
    e = [(int(name[a]), int(name[b])) for a, b in e]
    e += [(b, a) for a, b in e[::3]]
    ei = np.array([a for a, _ in e], dtype=np.int32)
    ej = np.array([b for _, b in e], dtype=np.int32)
    return ei, ej


SHAPES = ("chain", "star", "cliques", "forest", "sparse")


def csr_of_edges(n, ei, ej, rng):
    """the graph as a condensed vector -- edges at distance 1, other pairs at 2 or -1 -- and as its hit list"""
    cond = np.where(rng.random(n * (n - 1) // 2) < 0.2, 2, -1).astype(np.int32)
    lo, hi = np.minimum(ei, ej).astype(np.int64), np.maximum(ei, ej).astype(np.int64)
    cond[n * lo - lo * (lo + 1) // 2 + (hi - lo - 1)] = 1
    i, j = np.triu_indices(n, 1)
    keep = cond != -1
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i[keep], minlength=n), out=off[1:])
    return cond, off, j[keep].astype(np.int32), cond[keep].astype(np.int32)


# ---- the model

def closure_labels(n, adj):
    reach = adj | np.eye(n, dtype=bool)
    for _ in range(n):
        reach = reach | ((reach.astype(np.int32) @ reach.astype(np.int32)) > 0)
    return np.array([int(np.flatnonzero(reach[x])[0]) for x in range(n)], dtype=np.int32)


def reference_labels(n, i, j):
    """the smallest index of every vertex's component, by scipy where it imports, else by a transitive closure"""
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        assert n <= 60
        adj = np.zeros((n, n), dtype=bool)
        adj[i, j] = adj[j, i] = True
        return closure_labels(n, adj)
    _, comp = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32)


def assert_rules(m, n):
    """what the header promises of a result, whatever the graph"""
    label, size, off, mem = m["label"], m["componentSize"], m["componentOffsets"], m["members"]
    assert label.dtype == size.dtype == off.dtype == mem.dtype == np.int32
    assert label.shape == size.shape == mem.shape == (n,)
    assert np.all(label <= np.arange(n)) and np.array_equal(label[label], label)        # the label is a member, and a root
    roots = np.flatnonzero(label == np.arange(n))
    assert m["numComponents"] == len(roots) and off.shape == (len(roots) + 1,)
    assert np.array_equal(size, np.bincount(label, minlength=n)[label] if n else size)
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) > 0)
    assert sorted(mem.tolist()) == list(range(n))
    for c, r in enumerate(roots):                                     # components by label ascending, members ascending
        part = mem[off[c]:off[c + 1]]
        assert part[0] == r and np.all(label[part] == r) and np.all(np.diff(part) > 0)


@pytest.mark.parametrize("n", [0, 1, 2, 17, 60])
def test_model_against_reference(n):
    import edlib_amd
    rng = np.random.default_rng(100 + n)
    for level in (-1, 0, 1, 2):
        cells = n * (n - 1) // 2
        cond = rng.choice(np.array([-1, -1, -1, -1, -1, -1, 0, 1, 2, 3], dtype=np.int32), size=cells)
        i, j = np.triu_indices(n, 1)
        keep = cond != -1
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(i[keep], minlength=n), out=off[1:])
        m = edlib_amd.self_components_model(n, off, j[keep], cond[keep], level)
        edge = (cond >= 0) & ((cond <= level) if level >= 0 else True)
        assert np.array_equal(m["label"], reference_labels(n, i[edge], j[edge])), level
        assert_rules(m, n)
        # the same from the whole triangle, -1 entries included
        tri = np.concatenate([[0], np.cumsum(np.arange(n - 1, -1, -1))]).astype(np.int64) if n else np.zeros(1, dtype=np.int64)
        m2 = edlib_amd.self_components_model(n, tri, j, cond, level)
        for f in m:
            assert np.array_equal(m[f], m2[f]), f


def test_model_small_cases_by_hand():
    import edlib_amd
    # 0 -1- 3, 1 -2- 2, 4 alone; pairs by row
    off, partner, ed = [0, 1, 2, 2, 2, 2], [3, 2], [1, 2]
    m = edlib_amd.self_components_model(5, off, partner, ed, 2)
    assert m["label"].tolist() == [0, 1, 1, 0, 4] and m["componentSize"].tolist() == [2, 2, 2, 2, 1]
    assert m["numComponents"] == 3 and m["componentOffsets"].tolist() == [0, 2, 4, 5] and m["members"].tolist() == [0, 3, 1, 2, 4]
    m = edlib_amd.self_components_model(5, off, partner, ed, 1)
    assert m["label"].tolist() == [0, 1, 2, 0, 4] and m["numComponents"] == 4
    assert m["members"].tolist() == [0, 3, 1, 2, 4] and m["componentOffsets"].tolist() == [0, 2, 3, 4, 5]
    assert edlib_amd.self_components_model(5, off, partner, ed, 0)["numComponents"] == 5
    assert np.array_equal(edlib_amd.self_components_model(5, off, partner, ed, -1)["label"], [0, 1, 1, 0, 4])


# ---- the device code on the host

@pytest.mark.parametrize("shape", SHAPES)
def test_union_find_orders_and_threads(host, shape):
    rng = np.random.default_rng(SHAPES.index(shape))
    for n in (1, 2, 3, 7, 64, 65, 150, 300):
        ei, ej = graph(rng, n, shape)
        want = serial_labels(n, ei, ej)
        if shape in ("chain", "star") or (shape == "cliques" and n <= 9):
            assert not want.any()                                   # one component, labelled 0
        for _ in range(3):
            order = rng.permutation(len(ei))
            si, sj = np.ascontiguousarray(ei[order]), np.ascontiguousarray(ej[order])
            for threads in (1, 2, 8):
                got = np.full(n, -1, dtype=np.int32)
                assert host.self_components_host_edges(n, si.ctypes.data, sj.ctypes.data, len(si), threads, got.ctypes.data) == 0
                assert np.array_equal(got, want), (n, threads)


@pytest.mark.parametrize("shape", SHAPES)
def test_hit_list_and_dense_forms(host, shape):
    """the edges found from a CSR list (the row by the search of the offsets, empty rows between) and from the condensed
    vector, at level 1 between pairs at distance 2 and unreported pairs; and every pair at level -1 and 2"""
    import edlib_amd
    rng = np.random.default_rng(50 + SHAPES.index(shape))
    for n in (1, 2, 7, 65, 150):
        ei, ej = graph(rng, n, shape)
        cond, off, partner, ed = csr_of_edges(n, ei, ej, rng)
        for level in (1, 2, -1, 0):
            want = edlib_amd.self_components_model(n, off, partner, ed, level)["label"]
            if level == 1:
                assert np.array_equal(want, serial_labels(n, ei, ej))
            if level == 0:
                assert np.array_equal(want, np.arange(n))
            for threads in (1, 8):
                got = np.full(n, -1, dtype=np.int32)
                assert host.self_components_host_dense(n, cond.ctypes.data, level, threads, got.ctypes.data) == 0
                assert np.array_equal(got, want), (n, level, threads, "dense")
                order = rng.permutation(len(partner)).astype(np.int64)
                for o in (None, order.ctypes.data):
                    got[:] = -1
                    assert host.self_components_host_hits(n, off.ctypes.data, partner.ctypes.data, ed.ctypes.data,
                                                          len(partner), level, o, threads, got.ctypes.data) == 0
                    assert np.array_equal(got, want), (n, level, threads, "hits")


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_sanitizer_builds_run_clean(sanitize):
    """the same source with its own main(), as a child process: -fsanitize=address,undefined, and -fsanitize=thread"""
    tag = "tsan" if sanitize == "thread" else "san"
    exe = os.path.join(ROOT, "build", "self_components_host_" + tag)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (the runtimes linked into the program: it runs whatever else the loader brings in front of it)
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitize]
    flags += ["-static-libtsan"] if sanitize == "thread" else ["-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    if _stale(exe):
        # does the toolchain link these runtimes at all?  A trivial program says; the real source must then build
        probe = os.path.join(ROOT, "build", "sanitizer_probe_" + tag)
        r = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("the compiler here does not link the sanitizer runtimes: " + r.stderr.strip()[-200:])
        r = subprocess.run([probe], capture_output=True, text=True)
        if r.returncode != 0:                                         # (the thread sanitizer refuses some address layouts)
            pytest.skip("the sanitizer runtime does not start here: " + r.stderr.strip()[-200:])
        r = subprocess.run(["g++"] + flags + ["-DSELF_COMPONENTS_MAIN", "-o", exe, SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "WARNING: ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
