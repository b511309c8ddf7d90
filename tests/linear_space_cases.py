"""Deterministic inputs for the linear-space NW path (Batch::solvePaths / hirschbergLevel, hirschberg_split_kernel,
split_min_*, the known-split hand-over): the smallest shapes that still meet the 1 MiB rule, shared by the CPU model test
and the GPU test.  A case is (name, query, target, mode, eq_pairs); the name's first part is its group.

Every stream comes from numpy's legacy RandomState, whose output is frozen, and the fixture records the sha256 of every
sequence, so an input that drifted is noticed."""
import functools
import hashlib
import json
import os

import numpy as np

from linear_space_model import cigar_to_ops, first_T, needs_rule

IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
RULE_M = (64, 128, 320, 1000, 3000, 4096)                 # 1, 2, 5, 16, 47 and 64 blocks
RULE_T_FIRST = (37450, 21846, 9710, 3197, 1107, 815)
NO_MODEL = ("known_split/period5",)                       # a plain DP of 16,400 x 21,000 is too slow for the suite

# the score classes of a packed level's ring groups (ring_max_k of 4, 8, 16, 21, 32 and 64 lanes; beyond them the 64-lane
# ring holds queries of up to 64 blocks whole, and the wide band takes the rest)
PACKED_CAPS = (196, 456, 976, 1301, 2016, 4031)
PACKED_CLASSES = 8
PACKED_PAIRS = 288


def rand(rs, alphabet, n):
    return np.frombuffer(alphabet, dtype=np.uint8)[rs.randint(0, len(alphabet), n)].tobytes()


def periodic(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def edited(rs, src, edits, alphabet=b"ACGT", dele=0.3, ins=0.3):
    """`src` after `edits` scattered operations: deletions, insertions and substitutions in the given shares."""
    q = bytearray(src)
    for _ in range(edits):
        p = int(rs.randint(0, len(q)))
        x = rs.random_sample()
        if x < dele and len(q) > 1:
            del q[p]
        elif x < dele + ins:
            q.insert(p, alphabet[int(rs.randint(0, len(alphabet)))])
        else:
            others = [c for c in alphabet if c != q[p]]
            q[p] = others[int(rs.randint(0, len(others)))]
    return bytes(q)


def group(name):
    return name.split("/")[0]


def _rule_boundary():
    out = []
    for m, want in zip(RULE_M, RULE_T_FIRST):
        T1 = first_T(m)
        assert T1 == want and needs_rule(m, T1) and not needs_rule(m, T1 - 1), (m, T1, want)
        for side, T in (("first", T1), ("below", T1 - 1)):
            rs = np.random.RandomState(7000 + m)          # (the two sides share a prefix: one column apart)
            rq, rt = rand(rs, b"ACGT", m), rand(rs, b"ACGT", T1)
            out.append(("rule/m%d/%s/polyA" % (m, side), b"A" * m, b"A" * T, "NW", None))
            out.append(("rule/m%d/%s/period3" % (m, side), periodic(b"ACG", m), periodic(b"ACG", T), "NW", None))
            out.append(("rule/m%d/%s/random" % (m, side), rq, rt[:T], "NW", None))
    return out


def _boundary_rows():
    rs = np.random.RandomState(7101)
    q = rand(rs, b"ACG", 300)
    a, b = rand(rs, b"ACG", 2000), rand(rs, b"ACG", 3700)
    right = b"T" * 6000 + a + q + b
    return [
        ("rows/right", q, right, "NW", None),
        ("rows/left", q[::-1], right[::-1], "NW", None),
        ("rows/one_row", b"C", rand(rs, b"ACGT", 40000), "NW", None),
        ("rows/deep_right", q, b"T" * 41000 + q + b"T" * 6700, "NW", None),
        ("rows/deep_mid", q, b"T" * 23900 + q[:100] + b"T" * 50 + q[100:] + b"T" * 23750, "NW", None),
    ]


def _ties():
    rs = np.random.RandomState(7102)
    return [
        ("ties/polyA", b"A" * 1000, b"A" * 3300, "NW", None),
        ("ties/period3", periodic(b"ACG", 1000), periodic(b"ACG", 3301), "NW", None),
        ("ties/period5", periodic(b"ACGTT", 3000), periodic(b"ACGTT", 9000), "NW", None),
        ("ties/unrelated", rand(rs, b"ACGT", 1000), rand(rs, b"ACGT", 3300), "NW", None),
    ]


def _tall():
    rs = np.random.RandomState(7103)
    q = rand(rs, b"ACGT", 52400)
    t = rand(rs, b"ACGT", 65)
    assert needs_rule(52400, 64)
    return [("tall/T64", q, t[:64], "NW", None), ("tall/T65", q, t, "NW", None)]


def _similar():
    rs = np.random.RandomState(7104)
    t = rand(rs, b"ACGT", 9000)
    return [("similar/9000", edited(rs, t, 450), t, "NW", None)]


def _alphabets():
    rs = np.random.RandomState(7105)
    pt = rand(rs, PROTEIN, 3300)
    pq = pt[400:900] + pt[2100:2600]
    it = rand(rs, b"ACGTRYN", 3300)
    iq = bytearray(it[1100:2100])
    for p in rs.randint(0, 1000, 150):
        iq[p] = b"ACGTRYN"[int(rs.randint(0, 7))]
    dt = rand(rs, b"ACGT", 3300)
    dq = bytearray(dt[500:1500])
    for p in rs.randint(0, 1000, 60):
        dq[p] = b"NU-"[int(rs.randint(0, 3))]
    return [
        ("alpha/protein", pq, pt, "NW", None),
        ("alpha/iupac", bytes(iq), it, "NW", IUPAC),
        ("alpha/foreign_bytes", bytes(dq), dt, "NW", None),
    ]


def _known_split():
    # distance 4,600: beyond the widest ring's 4,031, and the shorter side is at least 16,384
    return [("known_split/period5", periodic(b"ACGTT", 16400), periodic(b"ACGTT", 21000), "NW", None)]


def _semi_global():
    rs = np.random.RandomState(7106)
    t = rand(rs, b"ACGT", 20000)
    q = edited(rs, t[9000:12000], 120)
    unit = rand(rs, b"ACGT", 7)
    pt = periodic(unit, 20000)
    pq = edited(rs, pt[9000:12000], 120)
    return [
        ("semi/hw_random", q, t, "HW", None),
        ("semi/hw_period7", pq, pt, "HW", None),
        ("semi/shw_random", q, t[9000:], "SHW", None),
    ]


@functools.lru_cache(maxsize=None)
def named_cases():
    cases = (_rule_boundary() + _boundary_rows() + _ties() + _tall() + _similar() + _alphabets() + _known_split()
             + _semi_global())
    assert len({c[0] for c in cases}) == len(cases)
    return tuple(cases)


def window(case, start, end):
    """The stretch of the target that the path of a case covers, from its first start and end location; the builder's
    promise that a semi-global case is inside the regime is asserted here."""
    name, q, t, mode, _ = case
    if mode == "NW":
        assert start == 0 and end == len(t) - 1
    w = t[start:end + 1]
    assert group(name) != "semi" or needs_rule(len(q), len(w)), (name, len(q), len(w))
    return w


# ------------------------------------------------------------------ the packed batch

# (scattered edits, random bases appended) of the ~3300 x 3300 copies, aimed at distances of about 60, 150, 300, 400, 700,
# 850, 1100, 1200, 1600 and 1900: scattered edits alone level off near 1,700, the distance of unrelated sequences
PACKED_EDITS = ((60, 0), (150, 0), (320, 0), (430, 0), (820, 0), (1100, 0), (1500, 0), (1800, 0), (3500, 0), (3500, 350))


@functools.lru_cache(maxsize=None)
def packed_batch():
    """288 NW pairs that all meet the rule, so that one level holds 256 pieces or more; the kinds are interleaved in the
    batch order, so that the groups of a level gather pieces from all over it."""
    rs = np.random.RandomState(7200)
    qs, ts = [], []
    kinds = len(PACKED_EDITS) + 3
    for i in range(PACKED_PAIRS):
        kind = i % kinds
        if kind < len(PACKED_EDITS):
            t = rand(rs, b"ACGT", 3300)
            edits, tail = PACKED_EDITS[kind]
            q = edited(rs, t, edits, dele=0.15, ins=0.15) + rand(rs, b"ACGT", tail)
        else:
            m, T = ((5000, 5000), (4000, 9000), (4200, 9000))[kind - len(PACKED_EDITS)]
            q, t = rand(rs, b"ACGT", m), rand(rs, b"ACGT", T)
        assert needs_rule(len(q), len(t))
        qs.append(q)
        ts.append(t)
    return tuple(qs), tuple(ts)


def packed_class(m, distance):
    for c, cap in enumerate(PACKED_CAPS):
        if distance <= cap:
            return c
    return len(PACKED_CAPS) + (-(-m // 64) > 64)


def packed_classes(distances):
    """The class of every pair of the packed batch from the expected distances, with at least 8 pairs in each."""
    qs, _ = packed_batch()
    assert len(distances) == len(qs)
    cls = [packed_class(len(q), d) for q, d in zip(qs, distances)]
    counts = [cls.count(c) for c in range(PACKED_CLASSES)]
    assert min(counts) >= 8, counts
    return cls


# ------------------------------------------------------------------ the recorded answers

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_space_paths.json")


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/linear_space_paths.json (oracle/gen_linear_space_golden.py): the compiled reference's answers."""
    with open(FIXTURE) as f:
        return json.load(f)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def batch_digest(qs, ts):
    h = hashlib.sha256()
    for q, t in zip(qs, ts):
        h.update(b"%d,%d;" % (len(q), len(t)))
        h.update(q)
        h.update(t)
    return h.hexdigest()


def packed_with_answers():
    """(queries, targets, fixture entries, classes) of the packed batch."""
    qs, ts = packed_batch()
    fx = fixture()
    assert len(fx["packed"]) == len(qs) == PACKED_PAIRS and batch_digest(qs, ts) == fx["packed_inputs_sha256"]
    return qs, ts, fx["packed"], packed_classes([e["distance"] for e in fx["packed"]])


def expected(entry):
    """Every field of EdlibAlignResult of a named case as the fixture has it (the fields the GPU tests compare)."""
    ops = cigar_to_ops(entry["cigar"])
    assert len(ops) == entry["alignmentLength"]
    return {"status": 0, "editDistance": entry["editDistance"], "endLocations": entry["endLocations"],
            "startLocations": entry["startLocations"], "numLocations": len(entry["endLocations"]),
            "alignment": ops, "alignmentLength": entry["alignmentLength"], "alphabetLength": entry["alphabetLength"]}


def cases_with_answers(groups=None):
    """[(case, fixture entry)] of the named cases of the given groups (all by default); no case without an entry, no
    entry without a case, and every input is the one the answers were recorded for."""
    cases, entries = named_cases(), fixture()["cases"]
    assert len(cases) == len(entries)
    out = []
    for case, e in zip(cases, entries):
        assert case[0] == e["name"] and case[3] == e["mode"]
        assert sha(case[1]) == e["query_sha256"] and sha(case[2]) == e["target_sha256"], case[0]
        if groups is None or group(case[0]) in groups:
            out.append((case, e))
    assert out
    return out
