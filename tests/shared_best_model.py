"""CPU model of the shared running best of the dense HW read scan (ReadScanArgs::liveBest).

The target is cut into segments; every segment starts `warm` columns early from the fresh state (HW is shift-invariant:
2m - 1 columns reproduce the bottom-row scores of its own columns) and keeps, for its own columns, the record the kernel
keeps: the best score, the number of columns attaining it and the first `cap` of them (EDLIB_AMD_TRACK_SCORE).  On the GPU
the segments of a read run in any order and at any pace, publish an improved best with an atomic minimum and look at the
shared value every kLivePeriod columns.  Whatever the timing, the value a segment imports is the read's threshold or a score
that some column of the target reaches, so it is never below the read's minimum over the whole target.  The model takes
exactly that freedom and no more: a SCHEDULE gives every segment a list of (column, value) imports, value >= the true
minimum, applied before that column is scored -- lower than best: best = value and the record is cleared; equal or higher:
nothing.  The merge is merge_segments_kernel's.  tests/test_shared_best_model.py sets the merged result against the
textbook DP for adversarial and random schedules.
"""
import numpy as np

from delay_rows_model import dp_bottom_row

CAP = 16          # positions a (read, segment) record keeps (kLastLevelCap)
CAP_FINAL = 16    # positions a read reports before its list overflows


def plan(T, S):
    """segment length (a multiple of 16) and the number of segments that leaves, as plan_segments does"""
    seg_len = (-(-T // S) + 15) // 16 * 16
    return seg_len, -(-T // seg_len)


def segment_scores(query, target, c0, c1, warm):
    """bottom-row scores of the columns [c0, c1) from a fresh state `warm` columns early (rounded down to 16)"""
    cw = max(0, c0 - warm) // 16 * 16
    return dp_bottom_row(query, target[cw:c1])[c0 - cw:]


def scan_segment(scores, c0, start, imports, cap=CAP):
    """The record of one segment.  scores[i] is the score of column c0 + i, `start` the best it starts from, imports a list
    of (column, value): before column `column` is scored, a value below best replaces it and clears the record."""
    by_col = {}
    for col, v in imports:
        by_col.setdefault(int(col), []).append(int(v))
    best, cnt, pos = int(start), 0, []
    for i, sc in enumerate(scores):
        for v in by_col.get(c0 + i, ()):
            if v < best:
                best, cnt, pos = v, 0, []
        sc = int(sc)
        if sc <= best:
            if sc < best:
                best, cnt, pos = sc, 0, []
            if cnt < cap:
                pos.append(c0 + i)
            cnt += 1
    for col, v in imports:                                    # imports past the last column (a reload after the last hit)
        if int(col) >= c0 + len(scores) and int(v) < best:
            best, cnt, pos = int(v), 0, []
    return best, cnt, pos


def merge(records, cap=CAP, cap_final=CAP_FINAL):
    """merge_segments_kernel: least best among the segments that recorded something, their counts added, the first
    cap_final positions in ascending order, and whether the list is incomplete"""
    live = [r for r in records if r[1] > 0]
    if not live:
        return -1, 0, [], False
    b = min(r[0] for r in live)
    n, pos, ovf = 0, [], False
    for best, cnt, p in records:
        if cnt <= 0 or best != b:
            continue
        ovf = ovf or cnt > cap
        pos.extend(p[:cap])
        n += cnt
    return b, n, pos[:cap_final], ovf or n > cap_final


def run(query, target, S, schedule, start=None, warm=None, cap=CAP):
    """Merged result of a scan in S segments.  schedule[s] = imports of segment s; start = every segment's first best
    (default: the read's own threshold m, k = -1)."""
    m, T = len(query), len(target)
    warm = 2 * m - 1 if warm is None else warm
    start = m if start is None else start
    seg_len, S = plan(T, S)
    records = []
    for s in range(S):
        c0, c1 = s * seg_len, min(T, (s + 1) * seg_len)
        records.append(scan_segment(segment_scores(query, target, c0, c1, warm), c0, start, schedule.get(s, ()), cap))
    return merge(records, cap)


def textbook(query, target, threshold=None, cap_final=CAP_FINAL):
    """(best, count, first positions, overflow) straight from the DP's bottom row"""
    row = dp_bottom_row(query, target)
    b = int(row.min())
    if threshold is not None and b > threshold:
        return -1, 0, [], False
    pos = [int(x) for x in np.flatnonzero(row == b)]
    return b, len(pos), pos[:cap_final], len(pos) > cap_final
