#!/usr/bin/env python3
"""Known answers for the linear-space NW path: every case of tests/linear_space_cases.py through the compiled,
unmodified reference (oracle/_ref/libedlib_ref.so, built by oracle/Makefile) at task = path.

Writes tests/golden/linear_space_paths.json: per named case the sha256 of query and target, editDistance, start and end
locations, alignmentLength, alphabetLength and the extended CIGAR; for the 288-pair packed batch the sha256 of each op
string and its distance.  Recorded results only.   Run from the repo root:  python oracle/gen_linear_space_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import linear_space_cases as cases            # noqa: E402
from linear_space_model import ops_to_cigar   # noqa: E402
from oracle.oracle import load_ref            # noqa: E402

DST = os.path.join(ROOT, "tests", "golden", "linear_space_paths.json")


sha = cases.sha


def named_entry(ref, case):
    name, q, t, mode, eqs = case
    r = ref.align(q, t, mode, "path", -1, eqs)
    assert r["status"] == 0, name
    cases.window(case, r["startLocations"][0], r["endLocations"][0])
    return {"name": name, "mode": mode, "query_sha256": sha(q), "target_sha256": sha(t),
            "editDistance": r["editDistance"], "startLocations": r["startLocations"], "endLocations": r["endLocations"],
            "alignmentLength": r["alignmentLength"], "alphabetLength": r["alphabetLength"],
            "cigar": ops_to_cigar(r["alignment"])}


def packed_entries(ref):
    qs, ts = cases.packed_batch()
    out = []
    for q, t in zip(qs, ts):
        r = ref.align(q, t, "NW", "path", -1, None)
        assert r["status"] == 0
        out.append({"distance": r["editDistance"], "ops_sha256": sha(r["alignment"])})
    cases.packed_classes([e["distance"] for e in out])
    return out, cases.batch_digest(qs, ts)


def render(named, packed, digest):
    """The fixture's text: one entry per line, so that it stays small and a changed case is one changed line."""
    def lines(entries):
        return "[\n" + ",\n".join(json.dumps(e, sort_keys=True, separators=(",", ":")) for e in entries) + "\n]"
    return ('{"generator":"oracle/gen_linear_space_golden.py",\n"cases":%s,\n"packed_inputs_sha256":"%s",\n"packed":%s}\n'
            % (lines(named), digest, lines(packed)))


def main():
    ref = load_ref()
    assert ref is not None, "build oracle/_ref first (make -C oracle)"
    named = [named_entry(ref, c) for c in cases.named_cases()]
    packed, digest = packed_entries(ref)
    with open(DST, "w") as f:
        f.write(render(named, packed, digest))
    print("%d named cases, %d packed pairs, %d bytes" % (len(named), len(packed), os.path.getsize(DST)))


if __name__ == "__main__":
    main()
