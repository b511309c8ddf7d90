"""The batches of tests/test_gpu_wide_rows.py (tests/wide_rows_cases.py), checked by the reference alone, without a GPU: they
are only worth running if the targets have exactly 8 and 16 symbols, the full-height batches leave the last level its 4,096
slots, and the planted reads put to the kernels what the batches are there for -- windows at both ends of the target, more
end locations than a slot keeps, every residue of the column mod 4, and every symbol row of the layout at a matching
position of a read that is still open after the first level."""
import numpy as np
import pytest

import wide_rows_cases as WR
from wide_rows_cases import T

FULL_CASES = [(n, layout) for layout in WR.LAYOUTS for n in WR.WORDS_FULL] + \
             [(n, layout) for layout in ("base", "rows8") for n in WR.WORDS_LONG]


@pytest.mark.parametrize("layout", WR.LAYOUTS)
def test_targets_have_exactly_eight_and_sixteen_symbols(layout):
    for nwd in (1, 5, 12):
        t = WR.target(77 + nwd, layout, WR.window_length(nwd))
        assert len(t) == T and T % 16 != 0 and T >= 65536
        assert set(t.tolist()) == set(WR.ALPHABET[layout]) and len(set(t.tolist())) == WR.SYMS[layout]
        assert t[T - 1] in (ord("N"), ord("n"))                     # the masking reaches the last column
        w = WR.window_length(nwd)
        assert len({t[s:s + w].tobytes() for s in WR.COPY_AT}) == 1
        assert t[WR.TWICE_AT[0]:WR.TWICE_AT[0] + w].tobytes() == t[WR.TWICE_AT[1]:WR.TWICE_AT[1] + w].tobytes()
        assert WR.TWICE_AT[0] % 4 != WR.TWICE_AT[1] % 4


def test_lower_case_is_applied_once_per_position():
    t8 = WR.target(5100, "rows8", 100)
    t16 = WR.target(5100, "rows16", 100)
    assert not np.any((t16 >= ord("a")) & ~np.isin(t16, np.frombuffer(b"acgtn", dtype=np.uint8)))
    assert WR.handed_back()["target"].tobytes() != t8.tobytes()     # (cases do not share a target)


@pytest.mark.parametrize("nwd,layout", FULL_CASES)
def test_full_height_batch(nwd, layout):
    b = WR.full(nwd, layout)                                        # asserts the symbol count, the lengths and the open reads
    reads, t = b["reads"], b["target"]
    assert len(set(t.tolist())) == WR.SYMS[layout]
    ls = WR.lengths_full(nwd)
    assert {len(r) for r in reads} == set(ls) and set(range(32 * nwd - 31, 32 * nwd + 1)) <= set(ls)    # every pad
    nslots = (len(reads) + 63) // 64 * 64
    assert 4096 <= b["open"] <= len(reads) and nslots < 16384, (b["open"], len(reads))
    for r in reads:
        if not set(r.tolist()) <= set(b"ACGT"):
            break
    else:
        assert layout == "base"                                     # planted reads carry the target's other symbols

    planted = [reads[p] for p in b["planted"]]
    ref = WR.reference(planted, t, "path")
    ed, loc = ref["editDistance"], ref["locOff"]
    ends = [ref["ends"][loc[i]:loc[i + 1]] for i in range(len(planted))]
    starts = [ref["starts"][loc[i]:loc[i + 1]] for i in range(len(planted))]
    still_open = [i for i in range(len(planted)) if ed[i] > WR.K_FIRST]
    assert len(still_open) >= 32, len(still_open)
    # the window at column 0 and the windows ending at T - 1 .. T - 4, in reads the full-height level scans
    assert 0 in starts[0]
    for j in range(4):
        assert T - 1 - j in ends[1 + j], (j, ends[1 + j])
    if nwd > 1:
        # (one word: a window of 30 rows with 12 edits may stand closer to the first level's threshold than its own count)
        assert all(ed[i] > WR.K_FIRST for i in range(5)), ed[:5]
    # more end locations than a slot's 16 positions, at a distance the first level does not resolve
    assert ed[5] > WR.K_FIRST and len(ends[5]) > 16, (ed[5], len(ends[5]))
    assert {s + WR.window_length(nwd) - 1 for s in WR.COPY_AT} <= set(ends[5].tolist())
    # the window that stands twice, at different residues of the column mod 4
    assert ed[6] > WR.K_FIRST or nwd == 1
    assert {s + WR.window_length(nwd) - 1 for s in WR.TWICE_AT} <= set(ends[6].tolist())
    assert len({e % 4 for e in ends[6].tolist()}) >= 2
    # every residue of the end column mod 4, over the open planted reads
    assert {int(e) % 4 for i in still_open for e in ends[i]} == set(range(4))
    # every symbol of the target at a matching position of a planted read that is still open after the first level
    seen = set()
    for i in still_open:
        a = ref["alignment"][ref["alnOff"][i]:ref["alnOff"][i + 1]]
        seen |= WR.matched_symbols(planted[i], t, starts[i][0], ends[i][0], a)
    assert seen == set(t.tolist()), (sorted(set(t.tolist()) - seen))


def test_sixteen_row_batch_of_long_reads_and_handed_back_batch():
    b = WR.long_on_sixteen_rows()
    assert len(set(b["target"].tolist())) == 16 and {len(r) for r in b["reads"]} >= set(range(257, 385, 5))
    assert min(len(r) for r in b["reads"]) >= 257 and max(len(r) for r in b["reads"]) <= 384
    b = WR.handed_back()
    assert len(set(b["target"].tolist())) == 8
    ls = [len(r) for r in b["reads"]]
    assert {385, 448, 449, 512} <= set(ls) and min(ls) >= 385 and max(ls) <= 512
    # unrelated reads at both lengths of either group: nothing the piece filter could narrow
    unrelated = [r for r in b["reads"] if len(r) in (385, 448, 449, 512)][:40]
    ed = WR.reference(unrelated, b["target"], "distance")["editDistance"]
    assert np.count_nonzero(ed > 100) >= 30


@pytest.mark.parametrize("layout", WR.LAYOUTS)
@pytest.mark.parametrize("nwd", WR.WORDS_FULL)
def test_banded_batch_spans_the_band_heights(nwd, layout):
    b = WR.banded(nwd, layout)
    reads, t = b["reads"], b["target"]
    assert len(set(t.tolist())) == WR.SYMS[layout]
    assert 300 <= len(reads) <= 500 and {32 * nwd - len(r) for r in reads} == set(range(32))
    ed = WR.reference(reads, t, "distance")["editDistance"]
    m = np.array([len(r) for r in reads])
    assert np.count_nonzero(ed <= WR.K_FIRST) >= 20                 # resolved by the first pass
    open_ = ed > WR.K_FIRST
    assert np.count_nonzero(open_) >= (3 if nwd == 1 else 100)       # the last level: far fewer than 4,096 (one word: every
    #                                                                   read of up to about 28 rows is within 8 of some column)
    if nwd >= 2:
        # distances from just above the first threshold to unrelated: a band of one word and a band of all of them
        assert np.any(open_ & (ed <= 16)) and np.any(ed * 10 >= m * 3)
    # reads hold the target's other symbols
    assert sum(1 for r in reads if not set(r.tolist()) <= set(b"ACGT")) >= 50
