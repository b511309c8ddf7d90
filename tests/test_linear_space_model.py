"""The linear-space NW path, without a GPU: the plain model of tests/linear_space_model.py reproduces the compiled
reference's op string on every case of tests/linear_space_cases.py that it can afford, the committed fixture is what the
reference gives, and a census pins which branches of the split search each input takes, so that an input cannot
silently stop exercising what it is for.  Every comparison is exact."""
import pytest

import linear_space_cases as C
import linear_space_model as M

GROUPS = ("rule", "rows", "ties", "tall", "similar", "alpha", "semi")


@pytest.fixture(scope="module")
def modelled(ref, oracle):
    """{name: (ops, census)} of every case with a model run; leaves through the compiled reference where it is built,
    through the C99 restatement otherwise (a leaf is below the rule, which both restate)."""
    impl = ref if ref is not None else oracle
    out = {}
    for case, e in C.cases_with_answers():
        name, q, t, _, eqs = case
        if name in C.NO_MODEL:
            continue
        w = C.window(case, e["startLocations"][0], e["endLocations"][0])
        out[name] = M.path(q, w, e["editDistance"], M.leaf_of(impl, eqs), eqs)
    return out


def test_the_rule_restated():
    assert tuple(M.first_T(m) for m in C.RULE_M) == C.RULE_T_FIRST == (37450, 21846, 9710, 3197, 1107, 815)
    for m, T in zip(C.RULE_M, C.RULE_T_FIRST):
        assert M.needs_rule(m, T) and not M.needs_rule(m, T - 1)
        assert (20 * ((m + 63) // 64) + 8) * T >= 2 ** 20 > (20 * ((m + 63) // 64) + 8) * (T - 1)
    assert M.needs_rule(1, 37450) and not M.needs_rule(65, 21845) and M.needs_rule(65, 21846)


def test_last_column_against_the_full_matrix():
    """the column-at-a-time recurrence against the textbook matrix filled cell by cell, equalities included"""
    import numpy as np
    rs = np.random.RandomState(5)
    for m, T, eqs in ((0, 5, None), (7, 0, None), (9, 13, None), (30, 17, C.IUPAC), (1, 40, None)):
        q, t = C.rand(rs, b"ACGTRYN", m), C.rand(rs, b"ACGTRYN", T)
        eq = M.equality_table(eqs)
        D = [[0] * (T + 1) for _ in range(m + 1)]
        for i in range(m + 1):
            for j in range(T + 1):
                if i == 0 or j == 0:
                    D[i][j] = i + j
                else:
                    D[i][j] = min(D[i - 1][j - 1] + (not eq[q[i - 1], t[j - 1]]), D[i - 1][j] + 1, D[i][j - 1] + 1)
        assert M.last_column(q, t, eq).tolist() == [row[T] for row in D]


def test_cigar_text_round_trip():
    ops = bytes([0, 0, 3, 1, 1, 2, 0])
    assert M.ops_to_cigar(ops) == "2=1X2I1D1=" and M.cigar_to_ops("2=1X2I1D1=") == ops
    assert M.ops_to_cigar(b"") == "" and M.cigar_to_ops("") == b""
    assert M.cigar_to_ops("12D") == bytes([2]) * 12


def test_validator_rejects_wrong_paths():
    q, t = b"ACGT", b"AGGTT"
    good = bytes([0, 3, 0, 0, 2])
    M.assert_path_valid(q, t, good, 2)
    for ops, ed in ((good, 3), (bytes([0, 0, 0, 0, 2]), 1), (bytes([3, 3, 0, 0, 2]), 3), (good[:-1], 1), (good + b"\x01", 3)):
        with pytest.raises(AssertionError):
            M.assert_path_valid(q, t, ops, ed)
    M.assert_path_valid(b"R", b"A", bytes([0]), 0, C.IUPAC)
    with pytest.raises(AssertionError):
        M.assert_path_valid(b"R", b"A", bytes([0]), 0)


@pytest.mark.parametrize("grp", GROUPS)
def test_model_reproduces_the_fixture(modelled, grp):
    """model ops == fixture (== the compiled reference, next test), and they are a valid path of that cost"""
    for case, e in C.cases_with_answers((grp,)):
        name, q, _, _, eqs = case
        ops, _ = modelled[name]
        assert M.ops_to_cigar(ops) == e["cigar"], name
        assert len(ops) == e["alignmentLength"], name
        M.assert_path_valid(q, C.window(case, e["startLocations"][0], e["endLocations"][0]), ops, e["editDistance"], eqs)


def test_known_split_case_is_a_valid_path():
    """the one case without a model run: fixture and validator only"""
    (case, e), = C.cases_with_answers(("known_split",))
    assert case[0] in C.NO_MODEL and e["editDistance"] == 4600 > C.PACKED_CAPS[-1] and min(len(case[1]), len(case[2])) >= 16384
    M.assert_path_valid(case[1], case[2], M.cigar_to_ops(e["cigar"]), e["editDistance"])


def test_fixture_is_what_the_reference_gives(ref):
    """every case, the packed batch included, through the compiled reference: the entries and the file's very bytes"""
    if ref is None:
        pytest.skip("oracle/_ref is not built here")
    from oracle import gen_linear_space_golden as gen
    fx = C.fixture()
    named = []
    for case, e in C.cases_with_answers():
        named.append(gen.named_entry(ref, case))
        assert named[-1] == e, case[0]
    packed, digest = gen.packed_entries(ref)
    assert digest == fx["packed_inputs_sha256"]
    assert packed == fx["packed"]
    with open(C.FIXTURE) as f:
        assert f.read() == gen.render(named, packed, digest)


def test_packed_batch_fills_every_class():
    qs, ts, entries, cls = C.packed_with_answers()
    assert len(qs) == 288 and all(M.needs_rule(len(q), len(t)) for q, t in zip(qs, ts))
    assert sorted(set(cls)) == list(range(C.PACKED_CLASSES))
    # interleaved, not grouped: no class is one contiguous run of the batch order
    for c in range(C.PACKED_CLASSES):
        at = [i for i, x in enumerate(cls) if x == c]
        assert at[-1] - at[0] + 1 > len(at), c
    # and the first 255 pairs (the batch below the packing threshold) still hold every class
    assert sorted(set(cls[:255])) == list(range(C.PACKED_CLASSES))


ROWS_CENSUS = {
    "rows/right": {"interior": 0, "top": 1, "bottom": 0, "empty_query_piece": 1, "depth": 1},
    "rows/left": {"interior": 0, "top": 0, "bottom": 1, "empty_query_piece": 1, "depth": 1},
    "rows/one_row": {"interior": 0, "top": 1, "bottom": 0, "empty_query_piece": 1, "depth": 1},
    "rows/deep_right": {"interior": 0, "top": 2, "bottom": 1, "empty_query_piece": 3, "depth": 3},
    "rows/deep_mid": {"interior": 1, "top": 1, "bottom": 2, "empty_query_piece": 3, "depth": 3},
}


def test_census_of_the_boundary_rows(modelled):
    assert sorted(ROWS_CENSUS) == sorted(c[0] for c, _ in C.cases_with_answers(("rows",)))
    for name, want in ROWS_CENSUS.items():
        census = modelled[name][1]
        assert {k: census[k] for k in want} == want, (name, census)


def test_census_of_ties_levels_and_regime(modelled):
    for case, _ in C.cases_with_answers(("ties",)):
        assert modelled[case[0]][1]["interior_tie"] >= 1, case[0]
    ties5 = modelled["ties/period5"][1]
    assert ties5["depth"] >= 3 and ties5["interior_tie"] >= 2, ties5          # ties on two levels
    similar = modelled["similar/9000"][1]
    assert similar["depth"] >= 3 and similar["interior"] == 7, similar
    # every case that is meant to be inside the regime splits at least once; every case below the rule never does
    for case, _ in C.cases_with_answers():
        name = case[0]
        if name in C.NO_MODEL:
            continue
        below = C.group(name) == "rule" and "/below/" in name
        assert (modelled[name][1]["depth"] == 0) == below, name


def test_rule_boundary_pairs_straddle_the_rule():
    by = {c[0]: (c, e) for c, e in C.cases_with_answers(("rule",))}
    assert len(by) == 36
    for m, T1 in zip(C.RULE_M, C.RULE_T_FIRST):
        for filling in ("polyA", "period3", "random"):
            (first, ef), (below, eb) = by["rule/m%d/first/%s" % (m, filling)], by["rule/m%d/below/%s" % (m, filling)]
            assert len(first[1]) == len(below[1]) == m and len(first[2]) == T1 and len(below[2]) == T1 - 1
            assert first[1] == below[1] and first[2][:-1] == below[2]
            assert M.needs_rule(m, len(first[2])) and not M.needs_rule(m, len(below[2]))
            if filling != "random":
                assert ef["cigar"] != eb["cigar"], (m, filling)
    # one column apart the walk of the stored matrix and the split give different paths (not just one column more)
    assert by["rule/m1000/below/polyA"][1]["cigar"] == "1000=2196D"
    assert by["rule/m1000/first/polyA"][1]["cigar"] == "1=1597D999=600D"


def test_leaves_agree_between_oracle_and_reference(ref, oracle, modelled):
    """the model's leaves through the C99 restatement and through the compiled reference give the same ops"""
    if ref is None:
        pytest.skip("oracle/_ref is not built here")
    for case, e in C.cases_with_answers(("rows", "ties", "tall", "alpha", "semi")):
        name, q, _, _, eqs = case
        w = C.window(case, e["startLocations"][0], e["endLocations"][0])
        ops, census = M.path(q, w, e["editDistance"], M.leaf_of(oracle, eqs), eqs)
        assert (ops, census) == modelled[name], name
