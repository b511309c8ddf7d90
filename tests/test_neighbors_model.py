"""CPU: the neighbour rules in numpy (edlib_amd.neighbors_model) against a brute force over random graphs with heavy ties,
and the device's selection schedule (edlib_amd/csrc/neighbors_core.hpp) run on the host over arrays of 64
(tests/neighbors_host.cpp: a program of its own, built with the address and undefined-behaviour sanitizers and run as a
child process)."""
import os
import subprocess

import numpy as np
import pytest

import edlib_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "neighbors_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "neighbors_core.hpp")


def brute(numRows, row, partner, distance, K, level):
    """the rule, one row at a time: the K smallest (distance, partner) among the row's candidates within the level"""
    count = np.zeros(numRows, dtype=np.int32)
    nb = np.full((numRows, K), -1, dtype=np.int32)
    dist = np.full((numRows, K), -1, dtype=np.int32)
    for r in range(numRows):
        cand = sorted((int(d), int(p)) for rr, p, d in zip(row, partner, distance)
                      if rr == r and d >= 0 and (level < 0 or d <= level))[:K]
        count[r] = len(cand)
        for x, (d, p) in enumerate(cand):
            nb[r, x], dist[r, x] = p, d
    return {"count": count, "neighbor": nb, "distance": dist}


def random_graph(rng, n, density, maxd):
    """a symmetric graph on n vertices as directed entries, distances in -1..maxd (so: heavy ties and pairs above k)"""
    i, j = np.triu_indices(n, 1)
    keep = rng.random(len(i)) < density
    i, j = i[keep], j[keep]
    d = rng.integers(-1, maxd + 1, size=len(i))
    order = rng.permutation(2 * len(i))
    return (np.concatenate([i, j])[order], np.concatenate([j, i])[order], np.concatenate([d, d])[order])


@pytest.mark.parametrize("n,density,maxd", [(1, 1.0, 2), (2, 1.0, 0), (7, 1.0, 1), (40, 0.3, 2), (90, 1.0, 3), (150, 0.05, 5)])
def test_model_equals_brute_force(n, density, maxd):
    rng = np.random.default_rng(n * 10 + maxd)
    row, partner, d = random_graph(rng, n, density, maxd)
    for K in (1, 2, 5, 63, 64):
        for level in (-1, 0, 1, maxd):
            got = edlib_amd.neighbors_model(n, row, partner, d, K, level)
            want = brute(n, row, partner, d, K, level)
            for f in ("count", "neighbor", "distance"):
                assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (f, K, level)


def test_model_on_rectangular_rows():
    """a cross batch's rows: targets x queries, the matrix flattened; rows without a candidate, no rows, no columns"""
    rng = np.random.default_rng(3)
    nt, nq = 9, 70
    m = rng.integers(-1, 3, size=(nt, nq))
    m[4] = -1
    t, q = np.divmod(np.arange(nt * nq), nq)
    for K in (1, 5, 64):
        for level in (-1, 0, 1):
            got = edlib_amd.neighbors_model(nt, t, q, m.reshape(-1), K, level)
            want = brute(nt, t, q, m.reshape(-1), K, level)
            for f in want:
                assert np.array_equal(got[f], want[f]), (f, K, level)
            assert got["count"][4] == 0 and np.all(got["neighbor"][4] == -1)
    empty = np.zeros(0, dtype=np.int64)
    got = edlib_amd.neighbors_model(0, empty, empty, empty, 3, -1)
    assert got["count"].shape == (0,) and got["neighbor"].shape == (0, 3)
    got = edlib_amd.neighbors_model(4, empty, empty, empty, 3, -1)
    assert got["count"].tolist() == [0] * 4 and np.all(got["distance"] == -1)


def test_model_first_columns_are_the_nearest_rules():
    """with every reported pair counted, columns 0 and 1 are self_nearest_model's nearest / nearestDistance / secondDistance"""
    rng = np.random.default_rng(11)
    n = 60
    i, j = np.triu_indices(n, 1)
    d = rng.integers(-1, 3, size=len(i))
    near = edlib_amd.self_nearest_model(n, i, j, d)
    got = edlib_amd.neighbors_model(n, np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([d, d]), 2, -1)
    assert np.array_equal(got["neighbor"][:, 0], near["nearest"])
    assert np.array_equal(got["distance"][:, 0], near["nearestDistance"])
    assert np.array_equal(got["distance"][:, 1], near["secondDistance"])


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


def test_host_schedule_runs_clean_under_sanitizers():
    """the schedule of neighbors_core.hpp over arrays of 64 against std::sort / std::partial_sort: random keys, all-equal
    distances, descending and ascending streams, streams of 1 .. 129 candidates, the condensed arithmetic; built with
    -fsanitize=address,undefined (without, where the toolchain links no sanitizer runtimes), as a child process"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "neighbors_host_san")
    # (the runtimes linked into the program: it runs whatever else the loader brings in front of it)
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan", "-static-libubsan"]
    if _stale(exe):
        probe = os.path.join(ROOT, "build", "sanitizer_probe")
        r = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
        if r.returncode != 0:
            flags = ["-O1", "-g", "-std=c++17"]
        r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout, r.stdout
