#!/usr/bin/env python3
"""The end of the last level's main launch: a CPU model of how the launch drains, and the same quantity taken
from the wave clocks of a diagnostic build.

  drain_model.py model [--reads 50400] [--T 5000000] [--jitter 0.15] [--seed 1]
      wall time of the launch with 84 uniform, 168 uniform and tapered segments against the ideal (all work at full rate)
  drain_model.py measure <clocks.bin> <out.json> [--label text]
      clocks.bin: the edlib_amd_drain.bin that a library built with -DEDLIB_AMD_DRAIN_DIAG added to the Makefile's HIPFLAGS leaves in the
      working directory (two uint64 gridX, gridY, then s_memrealtime of every wave at entry and at exit); a build with
      -DEDLIB_AMD_DRAIN_UNIFORM as well keeps the uniform plan, which is the parent's launch

Assumptions of the model (none of it is a GPU measurement):
  * 256 CUs x 8 workgroup slots (4 waves each, one per SIMD: r resident workgroups = r waves on every SIMD of the CU);
    workgroups start in order (segment-major: blockIdx.y slowest), each on the CU that frees a slot first.
  * A SIMD with r waves issues one instruction per CPI[r] cycles (tools/ifetch_ubench.hip at the scan's body size:
    1.96 / 2.02 / 2.09 / 2.16 / 2.23 / 2.28 / 2.35 / 4.45 cycles at 8 .. 1 waves), shared evenly by its waves.
  * A workgroup's work is (its segment's columns + the warm-up) x 56 ns of SIMD time per column at 8 waves, times a uniform
    jitter of +-15 % (with 1 % the launch runs in rounds, which the device does not show).
  * No memory stalls, no launch overhead, no clock changes.
The measurement prices the same way: the device's resident waves over 1,024 SIMDs give an average r(t); a SIMD at r waves
delivers CPI[8] / CPI[r] of its full rate (linear between whole r, nothing at 0); the loss is the integral of the shortfall
over the drain, i.e. from the last moment the launch holds its steady number of waves to its end.  The clocks do not say which SIMD a
wave ran on, so imbalance between CUs is averaged out: the priced loss is a lower bound of the real one.
"""
import argparse
import ctypes
import heapq
import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPI = {8: 1.96, 7: 2.02, 6: 2.09, 5: 2.16, 4: 2.23, 3: 2.28, 2: 2.35, 1: 4.45}
CUS, SLOTS, SIMDS = 256, 8, 1024
NS_PER_COLUMN = 56.0
TICK_NS = 10.0           # s_memrealtime counts at 100 MHz


def rel_rate(r):
    """rate of a SIMD holding r waves (fractional: the device's average) relative to 8 waves"""
    r = np.minimum(np.asarray(r, dtype=np.float64), 8.0)
    pts = np.array([0.0] + [CPI[8] / CPI[k] for k in range(1, 9)])
    return np.interp(r, np.arange(9), pts)


# ------------------------------------------------------------------------------------------------------------ the model

def planner():
    so = os.path.join(ROOT, "build", "libtapered_plan_host.so")
    src = os.path.join(ROOT, "tests", "tapered_plan_host.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def tapered_table(T, grid_x, resident, warm, lmax):
    lib = planner()
    out = (ctypes.c_int * (2 * 70000))()
    n = lib.plan_tapered_host(T, grid_x, resident, warm, lmax, out, 70000)
    return [out[2 * i + 1] for i in range(n)]


def simulate(seg_cols, grid_x, warm, jitter, seed):
    """wall time (ms) of a launch of grid_x workgroups per segment, segments in the given order, and the ideal"""
    rng = np.random.default_rng(seed)
    work = []
    for i, c in enumerate(seg_cols):
        w = (c + (warm if i else 0)) * NS_PER_COLUMN * 8.0            # ns of a workgroup alone among 8 at full rate
        work.extend((w * (1.0 + jitter * (2.0 * rng.random(grid_x) - 1.0))).tolist())
    total = sum(work)
    nxt = 0
    # per CU: virtual clock V (work done by each resident workgroup), heap of the finish values, time of the last update
    V = [0.0] * CUS; heaps = [[] for _ in range(CUS)]; last = [0.0] * CUS; ver = [0] * CUS
    speed = {r: (CPI[8] / CPI[r]) * 8.0 / r for r in range(1, 9)}   # progress of each of r workgroups per ns
    events = []

    def push(cu, now):
        ver[cu] += 1
        if heaps[cu]:
            heapq.heappush(events, (now + (heaps[cu][0] - V[cu]) / speed[len(heaps[cu])], cu, ver[cu]))

    for cu in range(CUS):
        for _ in range(SLOTS):
            if nxt < len(work):
                heapq.heappush(heaps[cu], work[nxt]); nxt += 1
    # (in-order start: slot s of every CU before slot s + 1 would interleave; the order within the first round does not matter)
    for cu in range(CUS):
        push(cu, 0.0)
    now = 0.0
    while events:
        t, cu, v = heapq.heappop(events)
        if v != ver[cu]:
            continue
        V[cu] += (t - last[cu]) * speed[len(heaps[cu])]; last[cu] = t; now = t
        heapq.heappop(heaps[cu])
        if nxt < len(work):
            heapq.heappush(heaps[cu], V[cu] + work[nxt]); nxt += 1
        push(cu, t)
    return now / 1e6, total / (CUS * SLOTS) / 1e6


def model(args):
    rblk = (args.reads + 63) // 64
    grid_x = (rblk + 3) // 4
    T, warm = args.T, args.warm
    rows = []
    for name, S in (("84 uniform", 84), ("168 uniform", 168)):
        seg = (T + S - 1) // S
        seg = (seg + 15) // 16 * 16
        cols = [min(seg, T - c) for c in range(0, T, seg)]
        rows.append((name, len(cols), simulate(cols, grid_x, warm, args.jitter, args.seed)))
    lmax = ((T + 83) // 84 + 15) // 16 * 16
    cols = tapered_table(T, grid_x, CUS * SLOTS, warm, lmax)
    rows.append(("tapered", len(cols), simulate(cols, grid_x, warm, args.jitter, args.seed)))
    for name, n, (wall, ideal) in rows:
        print("%-12s %4d segments: wall %.1f ms, ideal %.1f ms, lost %.1f ms" % (name, n, wall, ideal, wall - ideal))


# ------------------------------------------------------------------------------------------------------ the measurement

def measure(args):
    raw = open(args.clocks, "rb").read()
    gx, gy = struct.unpack_from("<QQ", raw, 0)
    nw = gx * gy * 4
    clk = np.frombuffer(raw, dtype=np.uint64, offset=16)
    assert len(clk) == 2 * nw, (len(clk), nw)
    entry, exit_ = clk[:nw].astype(np.int64), clk[nw:].astype(np.int64)
    ran = (entry > 0) & (exit_ > 0)
    entry, exit_ = entry[ran], exit_[ran]
    t0 = entry.min()
    e, x = (entry - t0) * TICK_NS / 1e6, (exit_ - t0) * TICK_NS / 1e6            # ms
    times = np.concatenate([e, x]); delta = np.concatenate([np.ones(len(e)), -np.ones(len(x))])
    order = np.argsort(times, kind="stable")
    times, resident = times[order], np.cumsum(delta[order])
    end = float(x.max())
    dt = np.diff(np.append(times, end))
    r = resident / SIMDS                                                          # average waves per SIMD
    # the steady level: the median of the resident waves between 10 % and 70 % of the launch (the dispatcher refills a freed
    # slot within microseconds, so the count sits a little under the capacity all along)
    mid = (times >= 0.1 * end) & (times <= 0.7 * end)
    full = float(np.median(resident[mid]))
    ok = np.nonzero(resident >= 0.99 * full)[0]
    i_ramp, i_drain = int(ok.min()), int(ok.max())                                # the drain: after the last moment at that level
    i_half = int(np.max(np.nonzero(resident >= 0.5 * full)[0]))
    seg = slice(i_drain, None)
    short = np.clip(1.0 - rel_rate(r) / rel_rate(full / SIMDS), 0.0, 1.0)         # shortfall against the steady level's rate
    priced = float(np.sum(short[seg] * dt[seg]))
    area = float(np.sum(np.clip(1.0 - resident[seg] / full, 0.0, 1.0) * dt[seg]))
    ramp = float(np.sum(short[:i_ramp] * dt[:i_ramp]))
    dur = x - e
    # the timeline, thinned: 64 points over the whole launch and 192 over its last 30 ms
    pick = np.unique(np.concatenate([np.searchsorted(times, np.linspace(0, end, 64), side="right") - 1,
                                     np.searchsorted(times, np.linspace(max(0.0, end - 30.0), end, 192), side="right") - 1]))
    pick = pick[pick >= 0]
    out = {
        "what": "resident waves of the last level's main launch against time, from s_memrealtime at every wave's entry and exit "
                "(diagnostic build, -DEDLIB_AMD_DRAIN_DIAG); losses priced with tools/drain_model.py's occupancy curve",
        "label": args.label, "grid": [int(gx) * 256, int(gy)], "waves_run": int(len(e)),
        "launch_ms": round(end, 3), "resident_waves_steady": int(full), "waves_per_simd_steady": round(full / SIMDS, 3), "resident_waves_max": int(resident.max()),
        "ramp_up_ms": round(float(times[i_ramp]), 3), "ramp_up_loss_ms": round(ramp, 3),
        "drain_starts_ms": round(float(times[i_drain]), 3), "drain_ms": round(end - float(times[i_drain]), 3),
        "below_half_ms": round(end - float(times[i_half]), 3),
        "drain_area_lost_ms": round(area, 3), "drain_loss_priced_ms": round(priced, 3),
        "wave_ms": {"min": round(float(dur.min()), 3), "median": round(float(np.median(dur)), 3), "max": round(float(dur.max()), 3)},
        "timeline_ms_waves": [[round(float(times[i]), 3), int(resident[i])] for i in pick],
    }
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("timeline_ms_waves", "what")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("model")
    m.add_argument("--reads", type=int, default=50400); m.add_argument("--T", type=int, default=5_000_000)
    m.add_argument("--warm", type=int, default=319); m.add_argument("--jitter", type=float, default=0.15)
    m.add_argument("--seed", type=int, default=1)
    s = sub.add_parser("measure")
    s.add_argument("clocks"); s.add_argument("out"); s.add_argument("--label", default="")
    a = ap.parse_args()
    {"model": model, "measure": measure}[a.cmd](a)
