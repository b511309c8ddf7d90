"""The flag logic of the merge and the gather of the exact pass (reads_kernels.hip: merge_segments_kernel,
gather_segments_kernel), restated in numpy (tests/overflow_cases.py) and held against a plain sort -- no GPU.  Random
per-segment records: counts past the cap, ties of the best score across segments, segments whose own best is worse."""
import numpy as np
import pytest

import overflow_cases as OC


def _lane(rng, S, seg_len, cap, crowd):
    """random hits of one lane: (columns ascending, scores); a few score levels so that ties across segments are common"""
    n = int(rng.integers(0, 4 * S if crowd else S))
    cols = np.sort(rng.choice(S * seg_len, n, replace=False)) if n else np.zeros(0, dtype=np.int64)
    scores = rng.integers(3, 6, len(cols))
    if crowd and n and rng.random() < 0.5:            # pile hits of the best score into one segment, past the cap
        g = int(rng.integers(0, S))
        extra = g * seg_len + rng.choice(seg_len, cap + int(rng.integers(1, 9)), replace=False)
        scores = np.where(np.isin(cols, extra), 3, scores)
        fresh = np.setdiff1d(extra, cols)
        order = np.argsort(np.concatenate([cols, fresh]), kind="stable")
        cols, scores = np.concatenate([cols, fresh])[order], np.concatenate([scores, np.full(len(fresh), 3)])[order]
    return cols, scores


@pytest.mark.parametrize("cap", [8, 16])
@pytest.mark.parametrize("crowd", [False, True])
def test_merge_and_gather_against_a_sort(cap, crowd):
    rng = np.random.default_rng(100 * cap + crowd)
    seen = {0: 0, 1: 0, 2: 0}
    for trial in range(600):
        S = int(rng.integers(1, 130))
        seg_len = int(rng.integers(2, 6)) * 16
        cols, scores = _lane(rng, S, seg_len, cap, crowd)
        best, cnt, pos = OC.segment_records(cols, scores, seg_len, S, cap)
        b, total, first, reason, gathered = OC.merge_gather(best, cnt, pos, cap)
        if len(cols) == 0:
            assert (b, total, reason) == (-1, 0, 0)
            continue
        want = [int(c) for c in cols[scores == scores.min()]]                    # the plain sort
        per_seg = np.bincount(np.asarray(want) // seg_len, minlength=S)
        assert b == scores.min() and total == len(want)                        # exact also past every cap
        assert reason == (1 if per_seg.max() > cap else (2 if len(want) > OC.CAP_FINAL else 0))
        assert reason == OC.reason_of(want, seg_len, cap)
        if reason == 0:
            assert first == want
        if reason != 1:
            assert first == want[:OC.CAP_FINAL]                                  # the slot's own 16 are the first 16
        if reason == 2:
            assert gathered == want                                              # complete and ascending, without a scan
        else:
            assert gathered is None
        seen[reason] += 1
    assert seen[0] > 0 and seen[2] > 0 and (seen[1] > 0) == crowd, seen


def test_a_short_list_crowded_into_one_segment_is_rescanned():
    """nine hits in one 8-position segment: the list would fit the slot's 16, but the segment dropped one"""
    cols = np.arange(9) * 3 + 64
    best, cnt, pos = OC.segment_records(cols, np.full(9, 7), 64, 4, 8)
    b, total, first, reason, gathered = OC.merge_gather(best, cnt, pos, 8)
    assert (b, total, reason, gathered) == (7, 9, 1, None) and first == list(cols[:8])
    assert OC.reason_of(cols, 64, 8) == 1 and OC.reason_of(cols, 64, 16) == 0
