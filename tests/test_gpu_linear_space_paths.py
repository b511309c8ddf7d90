"""-m gpu: EDLIB_TASK_PATH at and beyond the reference's 1 MiB rule (Batch::solvePaths / hirschbergLevel,
hirschberg_split_kernel, split_min_*, the known-split hand-over of solveWideSplit) on the inputs of
tests/linear_space_cases.py: lopsided pairs that take the two boundary answers of the split search and leave empty-query
pieces, low-complexity input whose every tie decides the CIGAR, pairs one column below and at the rule, levels of 256
pieces and more spread over every ring group, wider alphabets and equalities, HW / SHW windows inside the regime.

Expected values are the compiled reference's answers as committed in tests/golden/linear_space_paths.json (checked
against the reference and a plain model by tests/test_linear_space_model.py), so nothing here depends on the reference
having travelled; where it did, it is compared too.  Every comparison is exact: all result fields, the op string byte
for byte (by sha256 for the packed batch), and the ops must be a valid path of exactly that cost."""
import numpy as np
import pytest

import linear_space_cases as C
import linear_space_model as M
pytestmark = pytest.mark.gpu
FIELDS = ("status", "editDistance", "endLocations", "startLocations", "numLocations",        # (as in test_gpu_rings.py)
          "alignment", "alignmentLength", "alphabetLength")

_ref_answers = {}


def _ref_answer(ref, case):
    name, q, t, mode, eqs = case
    if name not in _ref_answers:
        _ref_answers[name] = ref.align(q, t, mode, "path", -1, eqs)
    return _ref_answers[name]


def _compare(got, case, entry, ref, what):
    name, q, t, _, eqs = case
    want = C.expected(entry)
    diff = {f: (got[f], want[f]) for f in FIELDS if got[f] != want[f] and f != "alignment"}
    assert not diff, (what, name, diff)
    assert got["alignment"] == want["alignment"], (what, name, M.ops_to_cigar(got["alignment"])[:200], entry["cigar"][:200])
    M.assert_path_valid(q, C.window(case, got["startLocations"][0], got["endLocations"][0]), got["alignment"],
                        got["editDistance"], eqs)
    if ref is not None:
        r = _ref_answer(ref, case)
        assert all(got[f] == r[f] for f in FIELDS), (what, name, "compiled reference")


def _batches(pairs):
    """the cases split by what one batch shares: mode and equalities"""
    keys = []
    for case, _ in pairs:
        key = (case[3], tuple(case[4] or ()))
        if key not in keys:
            keys.append(key)
    return [[(c, e) for c, e in pairs if (c[3], tuple(c[4] or ())) == key] for key in keys]


def _check_batched(engine, ref, pairs, what, count):
    """every case of `pairs` through align_pairs, one batch per mode and set of equalities"""
    assert len(pairs) == count
    done = 0
    for part in _batches(pairs):
        mode, eqs = part[0][0][3], part[0][0][4]
        got = engine.align_pairs([c[1] for c, _ in part], [c[2] for c, _ in part], mode=mode, task="path", k=-1,
                                 additionalEqualities=eqs, raw=True)
        assert len(got) == len(part)
        for g, (case, e) in zip(got, part):
            _compare(g, case, e, ref, what)
            done += 1
    assert done == count


@pytest.mark.parametrize("m", C.RULE_M)
def test_rule_boundary(engine, ref, m):
    """one column below the rule the path is the walk of the stored matrix, at the rule it is two halves joined at the
    first row that attains the score: 1, 2, 5, 16, 47 and 64 blocks, poly-A, period 3 and random"""
    pairs = [(c, e) for c, e in C.cases_with_answers(("rule",)) if c[0].startswith("rule/m%d/" % m)]
    _check_batched(engine, ref, pairs, "rule boundary", 6)
    for case, _ in pairs:
        assert M.needs_rule(len(case[1]), len(case[2])) == ("/first/" in case[0])


def test_boundary_rows(engine, ref):
    """the whole query goes right (i = -1) or left (i = m - 1), down to three levels, with the empty-query pieces"""
    _check_batched(engine, ref, C.cases_with_answers(("rows",)), "boundary rows", 5)


def test_ties(engine, ref):
    """thousands of rows attain the score: the first interior one is the reference's"""
    _check_batched(engine, ref, C.cases_with_answers(("ties",)), "ties", 4)


def test_tall_query_few_columns(engine, ref):
    """819 blocks over 64 and 65 columns (the odd T // 2)"""
    _check_batched(engine, ref, C.cases_with_answers(("tall",)), "tall", 2)


def test_similar_pairs_several_levels(engine, ref):
    _check_batched(engine, ref, C.cases_with_answers(("similar",)), "similar", 1)


def test_alphabets_and_equalities(engine, ref):
    """20 letters, IUPAC equalities, query bytes the target lacks"""
    _check_batched(engine, ref, C.cases_with_answers(("alpha",)), "alphabets", 3)


def test_known_split_with_ties(engine, ref, checker):
    """16,400 x 21,000 of period 5 at distance 4,600: the split found by the two half scans of the distance phase is
    handed to the path; alone, and inside a batch with two short pairs"""
    (case, e), = C.cases_with_answers(("known_split",))
    name, q, t, mode, eqs = case
    _compare(engine.align_raw(q, t, mode, "path", -1, eqs), case, e, ref, "known split, single call")
    rs = np.random.RandomState(7301)
    shorts = []
    for n in (90, 700):
        st = C.rand(rs, b"ACGT", n)
        shorts.append((C.edited(rs, st, n // 20), st))
    qs, ts = [shorts[0][0], q, shorts[1][0]], [shorts[0][1], t, shorts[1][1]]
    got = engine.align_pairs(qs, ts, mode="NW", task="path", k=-1, raw=True)
    assert len(got) == 3
    _compare(got[1], case, e, ref, "known split, in a batch")
    for i in (0, 2):
        want = checker.align(qs[i], ts[i], "NW", "path", -1)
        assert want["status"] == 0 and all(got[i][f] == want[f] for f in FIELDS), i


def test_semi_global_windows_in_the_regime(engine, ref):
    """HW (random and period-7 target: thousands of end locations) and SHW paths whose window meets the rule"""
    pairs = C.cases_with_answers(("semi",))
    for case, e in pairs:
        assert M.needs_rule(len(case[1]), e["endLocations"][0] - e["startLocations"][0] + 1)
    _check_batched(engine, ref, pairs, "semi-global", 3)


def _check_packed(got, qs, ts, entries, what, ref=None):
    assert len(got) == len(qs) == len(ts) == len(entries)
    bad = []
    for i, (g, q, t, e) in enumerate(zip(got, qs, ts, entries)):
        ok = (g["status"] == 0 and g["editDistance"] == e["distance"] and g["alignment"] is not None
              and C.sha(g["alignment"]) == e["ops_sha256"] and g["alignmentLength"] == len(g["alignment"])
              and g["startLocations"] == [0] and g["endLocations"] == [len(t) - 1] and g["numLocations"] == 1)
        if not ok:
            bad.append((i, len(q), len(t), g["status"], g["editDistance"], e["distance"]))
    assert not bad, (what, len(bad), bad[:5])
    for g, q, t in zip(got, qs, ts):
        M.assert_path_valid(q, t, g["alignment"], g["editDistance"])
    if ref is not None:
        for i, (g, q, t) in enumerate(zip(got, qs, ts)):
            r = ref.align(q, t, "NW", "path", -1)
            assert all(g[f] == r[f] for f in FIELDS), (what, i, "compiled reference")


def test_packed_levels(engine, ref):
    """288 pairs in one batch: every level holds 256 pieces or more, sorted into all seven ring groups by score and
    mapped back; the first 255 of them (one below the packing threshold); and one pair of each group alone"""
    qs, ts, entries, cls = C.packed_with_answers()
    got = engine.align_pairs(list(qs), list(ts), mode="NW", task="path", k=-1, raw=True)
    _check_packed(got, qs, ts, entries, "288 pairs", ref)
    got = engine.align_pairs(list(qs[:255]), list(ts[:255]), mode="NW", task="path", k=-1, raw=True)
    _check_packed(got, qs[:255], ts[:255], entries[:255], "255 pairs")
    # the groups of a packed level: six rings by score, the 64-lane ring also for any score on up to 64 blocks, the wide band
    singles = [cls.index(c) for c in (0, 1, 2, 3, 4, 6, 7)]
    assert len(set(singles)) == 7
    for i in singles:
        got = [engine.align_raw(qs[i], ts[i], "NW", "path", -1)]
        _check_packed(got, qs[i:i + 1], ts[i:i + 1], entries[i:i + 1], "single pair %d" % i)


def test_entry_points_and_repeats(engine, ref):
    """all named NW cases as one batch in a shuffled order, each alone through the single-call entry point, and a
    resident batch run twice with identical views"""
    pairs = [(c, e) for c, e in C.cases_with_answers() if c[3] == "NW"]
    plain = [(c, e) for c, e in pairs if c[4] is None]
    assert len(pairs) == len(C.named_cases()) - 3 and len(plain) == len(pairs) - 1
    order = np.random.RandomState(7300).permutation(len(plain))
    assert list(order) != sorted(order)
    shuffled = [plain[i] for i in order]
    _check_batched(engine, ref, shuffled, "shuffled batch", len(plain))
    for case, e in pairs:
        name, q, t, mode, eqs = case
        _compare(engine.align_raw(q, t, mode, "path", -1, eqs), case, e, ref, "single call")
    b = engine.PairBatch([c[1] for c, _ in shuffled], [c[2] for c, _ in shuffled], mode="NW", task="path", k=-1)
    try:
        b.run()
        first = b.results_flat()
        b.run()
        second = b.results_flat()
        for key in first:
            assert np.array_equal(first[key], second[key]), key
        for g, (case, e) in zip(b.results(raw=True), shuffled):
            _compare(g, case, e, None, "second run")
        aln = second["alnOff"]
        for i, (case, e) in enumerate(shuffled):
            assert second["alignment"][aln[i]:aln[i + 1]].tobytes() == C.expected(e)["alignment"], case[0]
    finally:
        b.close()
