"""-m gpu: the exact k-mer seed filter that replaces the banded first pass of HW read groups against a target of at most four
symbols (edlib_amd/csrc/reads_seed.hip; the argument is tests/seed_model.py).  Every batch is compared with
the reference on every field.  The batches that take the new path prove it through the work counter: the banded first pass
computes at least one word per column per read, so word_steps stays below nslots x T only when the seeds did the first pass.

The planted batches of tests/seed_cases.py pin what the kernel DOES, from the outside, with tests/seed_model.py as the
predictor: the word-steps of a seed pass that is the only level equal NWD x the columns of the model's merged windows (all
eight word counts; a false or a missed hit, a missed de-duplication, a wrong merge or clip changes the sum), and the library's
own EDLIB_AMD_DEBUG lines, read from a child process, give the threshold the engine chose (Batch::seedThreshold), the number
of reads each cap handed back (the model, caps on) and the number of reads the next level rescanned (the reads the reference
puts above the threshold: a read within it that the seed pass lost would be one more).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import seed_cases as SC
import seed_model as SM
from edlib_amd import synth
from oracle import oracle as O
from seed_cases import _mutate, _reads
from seed_model import seed_threshold
from test_gpu_long_reads import _check

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _nslots(n):
    return (n + 63) // 64 * 64


def test_seed_batch_a(engine):
    """16,384 reads of 129..160 bases against 256 kb: one group of five words"""
    target = synth.random_dna(801, 256_000)
    kf = seed_threshold(129, len(target))
    assert kf == 8
    reads = _reads(target, 16_384, 802, kf)
    reads[0] = np.ascontiguousarray(target[:129])                      # shortest and longest reads at both ends
    reads[1] = np.ascontiguousarray(target[-160:])
    reads[2] = np.ascontiguousarray(np.concatenate([_ACGT[[0, 1, 2]], target[:140]]))   # hanging over the first column
    reads[3] = np.ascontiguousarray(np.concatenate([target[-140:], _ACGT[[3, 2]]]))     # and over the last
    st = _check(engine, reads, target, "distance")
    assert st["path"] & 1
    assert st["word_steps"] < _nslots(len(reads)) * len(target), st


def test_seed_repeats_exact_pass_and_hand_back(engine):
    """a 150-base block copied 20 times (more than 16 end locations: the exact pass) and another copied 100 times (past the
    bucket cap: handed back to the banded scan)"""
    rng = np.random.default_rng(811)
    T = 256_000
    target = synth.random_dna(812, T).copy()
    blocks = [synth.random_dna(813, 150), synth.random_dna(814, 150)]
    starts = rng.choice(np.arange(0, T - 150, 160), 120, replace=False)
    for j, at in enumerate(starts):
        target[at:at + 150] = blocks[0 if j < 20 else 1]
    kf = seed_threshold(150, T)
    reads = _reads(target, 8_192, 815, kf, mlo=150, mhi=150, unrelated=0.02, above=0.0, with_n=0.0)
    for b in blocks:
        for e in range(6):
            reads.append(_mutate(rng, b, e, [int(x) for x in rng.integers(0, 150, 6)]) if e else np.ascontiguousarray(b))
    st = _check(engine, reads, target, "distance")
    assert st["overflow_units"] >= 1, st
    assert st["word_steps"] < _nslots(len(reads)) * T, st


@pytest.mark.parametrize("k", [3, 20])
def test_seed_caller_k(engine, k):
    target = synth.random_dna(821, 256_000)
    kf = seed_threshold(131, len(target))
    reads = _reads(target, 8_192, 822 + k, kf)
    st = _check(engine, reads, target, "distance", k=k)
    assert st["word_steps"] < _nslots(len(reads)) * len(target), st


def test_five_symbol_target_keeps_banded_pass(engine):
    """ACGTN: not the new path (more than four symbols); the banded first pass computes >= one word per column per read"""
    target = synth.random_dna(831, 256_000).copy()
    target[np.random.default_rng(832).integers(0, len(target), 300)] = ord("N")
    reads = _reads(target, 8_192, 833, seed_threshold(131, len(target)))
    st = _check(engine, reads, target, "distance")
    assert st["word_steps"] >= _nslots(len(reads)) * len(target), st


# ------------------------------------------------------------------------------------------ planted batches (seed_cases.py)

_FIELDS = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")


def _reference(b):
    reads = b["reads"]
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    return O.pool_align(np.concatenate(reads), qoff, b["target"], np.array([0, len(b["target"])], dtype=np.int64), True, "HW",
                        b["task"], b["k"])


def _account(engine, b, nwd):
    """the seed pass is the only level (the caller's k is its threshold), the model hands nothing back, no read has more than
    16 end locations: the work counter holds NWD word-steps per column of the model's merged windows and nothing else"""
    k = b["k"]
    m_min = min(len(r) for r in b["reads"])
    assert all((len(r) + 31) // 32 == nwd for r in b["reads"]) and 0 <= k <= seed_threshold(m_min, len(b["target"]))
    assert _nslots(len(b["reads"])) < 16_384 and _nslots(len(b["reads"])) * len(b["target"]) >= 1 << 30
    pred = SM.predict_batch(b["reads"], b["target"], k)
    assert sum(p["back"] for p in pred) == 0
    want = nwd * sum(p["columns"] for p in pred)
    st = _check(engine, b["reads"], b["target"], "distance", k=k)
    print("nwd=%d k=%d T=%d reads=%d: word_steps %d, model %d, diagonals per read %.4f"
          % (nwd, k, len(b["target"]), len(b["reads"]), st["word_steps"], want, sum(p["diagonals"] for p in pred) / len(pred)))
    assert st["overflow_units"] == 0, st
    assert st["word_steps"] == want, (st, want)


@pytest.mark.parametrize("nwd", range(1, 9))
def test_seed_work_is_the_models_windows(engine, nwd):
    """every word count at its k_f (T = 256,000 +- 1: k_f = 1 / 3 / 5 / 7 / 8 / 11 / 13 / 16): parity of every field, and
    word_steps == NWD x sum of the model's merged window lengths"""
    b = SC.single_group(nwd, seed_threshold(SC.M_MIN[nwd], 256_000), mlo=SC.M_MIN[nwd])
    assert b["k"] == (1, 3, 5, 7, 8, 11, 13, 16)[nwd - 1] == seed_threshold(SC.M_MIN[nwd], len(b["target"]))
    _account(engine, b, nwd)


@pytest.mark.parametrize("nwd,k", [(1, 0), (4, 0), (4, 1), (4, 6), (8, 0), (8, 1), (8, 15), (3, 1)])
def test_seed_work_at_small_k(engine, nwd, k):
    """k = 0 (one piece: the whole read, up to 256 symbols), 1 and k_f - 1 for one, four and eight words (reads from
    32 (NWD - 1) + 1 bases on); (3, 1): pieces of 43 and 44 symbols"""
    _account(engine, SC.single_group(nwd, k), nwd)


_SEED_LINE = re.compile(r"seed pass nwords=(\d+) k=(-?\d+): (\d+) of (\d+) slots handed back")
_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned")
_LADDER_LINE = re.compile(r"ladder nwords=(\d+) kFirst=(\d+) open=(\d+)/(\d+) levels:((?: \d+\([0-9.]+\))*) full")


def _child(name, tmp_path):
    """the batch SC.batch(name) in a fresh process with EDLIB_AMD_DEBUG=1: every field against the reference; returns the
    batch, the reference, the stats and the library's lines: {"seed": {nwords: (k, handed back, slots)}, "levels": {nwords:
    [slots rescanned, per level]}, "ladder": {nwords: (kFirst, [levels])}}"""
    out = str(tmp_path / "child.npz")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "seed_child.py"), name, out],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    log = {"seed": {}, "levels": {}, "ladder": {}}
    cur = None
    for line in p.stderr.splitlines():
        m = re.search(r"nwords=(\d+)", line)
        if m:
            cur = int(m.group(1))
        m = _SEED_LINE.search(line)
        if m:
            assert cur not in log["seed"]
            log["seed"][cur] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
        m = _LEVEL_LINE.search(line)
        if m:
            log["levels"].setdefault(cur, []).append(int(m.group(2)))
        m = _LADDER_LINE.search(line)
        if m:
            log["ladder"][cur] = (int(m.group(2)), [int(x) for x in re.findall(r" (\d+)\(", m.group(5))])
    b = SC.batch(name)
    got = np.load(out)
    ref = _reference(b)
    for f in _FIELDS:
        assert np.array_equal(got[f], ref[f]), (name, f)
    st = json.loads(str(got["stats"]))
    print(name, log, st)
    return b, ref, st, log


def _groups(b):
    """word count -> indices of its reads"""
    out = {}
    for i, r in enumerate(b["reads"]):
        out.setdefault((len(r) + 31) // 32, []).append(i)
    return out


def _handed_back(b, log):
    """per group: the seed pass ran at the expected threshold and handed back exactly the reads the model hands back"""
    T = len(b["target"])
    for nwd, idx in _groups(b).items():
        if nwd not in b["K"]:
            assert nwd not in log["seed"]
            continue
        K = b["K"][nwd]
        assert K <= seed_threshold(min(len(b["reads"][i]) for i in idx), T)
        pred = SM.predict_batch([b["reads"][i] for i in idx], b["target"], K)
        assert log["seed"][nwd] == (K, sum(p["back"] for p in pred), _nslots(len(idx))), (nwd, log["seed"])
    return True


@pytest.mark.parametrize("nwd", [1, 3, 5, 8])
def test_caps_on_both_sides(nwd, tmp_path):
    """32 diagonals, a bucket of 64 positions and a merged window of 1024 columns (at least four diagonals, scanned inside the
    kernel) are NOT handed back; 33, 65 and 1025 are: the library's own count against the model, parity of every field"""
    b, ref, st, log = _child("caps:%d" % nwd, tmp_path)
    pred = SM.predict_batch(b["reads"], b["target"], b["k"])
    assert SC.claims_hold(b["claims"], pred, keys=("back",)) == []
    caps = [(c, p) for c, p in zip(b["claims"], pred)
            if c and (c["back"] or c.get("bucket", 0) >= 64 or c.get("window") or c.get("diagonals", 0) >= 32)]
    assert len(caps) == 6 and SC.claims_hold([c for c, _ in caps], [p for _, p in caps]) == []
    assert 32 in {p["diagonals"] for _, p in caps} and {p["bucket"] for _, p in caps} >= {64, 65} and {p["window"] for _, p in caps} >= {1024, 1025}
    assert _handed_back(b, log) and log["seed"][nwd][1] >= 3
    assert not log["levels"], log                              # (the caller's k is k_f: no later level)


def test_k_minus_one_hides_no_false_negative(tmp_path):
    """groups of 4 .. 8 words against 200,000 columns, k = -1, one later level: the engine's thresholds are k_f of every
    group's shortest read, and the next level rescans exactly the reads the reference puts above it"""
    b, ref, st, log = _child("kminus1", tmp_path)
    T = len(b["target"])
    assert T == 200_000 and b["K"][4] == seed_threshold(108, T) == 8
    groups = _groups(b)
    assert sorted(groups) == [4, 5, 6, 7, 8] == sorted(log["seed"])
    for nwd, idx in groups.items():
        m_min = min(len(b["reads"][i]) for i in idx)
        assert m_min == SC.M_MIN[nwd] and 1_024 <= _nslots(len(idx)) < 16_384
        K = log["seed"][nwd][0]
        assert K == seed_threshold(m_min, T) == b["K"][nwd]
        above = int(np.sum(ref["editDistance"][idx] > K))
        assert above > 0 and log["levels"][nwd] == [above], (nwd, above, log["levels"])
    assert _handed_back(b, log)


@pytest.mark.parametrize("name", ["ineligible108", "five"])
def test_no_seed_pass_where_the_engine_must_not_take_one(name, tmp_path):
    """108-base reads against 256,000 columns (k_f = 7, below the banded pass's first threshold) at k = -1; a five-symbol
    target: no `seed pass` line, the banded pass computes at least a word per column per read"""
    b, ref, st, log = _child(name, tmp_path)
    if name == "ineligible108":
        assert min(len(r) for r in b["reads"]) == 108 and seed_threshold(108, len(b["target"])) == 7
    else:
        assert len(set(b["target"].tolist())) == 5
    assert not log["seed"], log
    assert st["word_steps"] >= _nslots(len(b["reads"])) * len(b["target"]), st


@pytest.mark.parametrize("task", ["locations", "path"])
@pytest.mark.parametrize("nwd", [5, 8])
def test_start_locations_and_paths_on_a_seed_pass(engine, nwd, task):
    """indels at both read ends, reads clipped at both target ends, every planted case: starts and alignments too"""
    b = SC.single_group(nwd, seed_threshold(SC.M_MIN[nwd], 256_000), mlo=SC.M_MIN[nwd], over_caps=True, many_locations=True,
                        task=task, seed=1)
    st = _check(engine, b["reads"], b["target"], task, k=b["k"])
    assert st["word_steps"] < _nslots(len(b["reads"])) * len(b["target"]), st


def test_four_seed_groups_in_permuted_order(engine):
    """2, 4, 6 and 8 words (k = 3: all eligible), 4,300 reads each in random unit order, and five 20-base reads (a group of
    their own on the banded pass): the gathered view and the per-unit records"""
    T = 256_000
    extra = [synth.random_dna(900 + i, 20) for i in range(5)]
    b = SC.several_groups((2, 4, 6, 8), {w: 3 for w in (2, 4, 6, 8)}, T, 4_300, 8200, 3, extra=extra)
    groups = _groups(b)
    assert sorted(groups) == [1, 2, 4, 6, 8]
    eligible = 0
    for nwd in (2, 4, 6, 8):
        assert seed_threshold(min(len(b["reads"][i]) for i in groups[nwd]), T) >= 3
        assert _nslots(len(groups[nwd])) >= 1_024 and _nslots(len(groups[nwd])) * T >= 1 << 30
        eligible += _nslots(len(groups[nwd])) * T
    B = engine.SharedBatch(b["reads"], b["target"], mode="HW", task="distance", k=3)
    try:
        st = B.run()
        got = B.results_flat()
        rec = B.results(raw=True)
    finally:
        B.close()
    ref = _reference(b)
    for f in _FIELDS:
        assert np.array_equal(got[f], ref[f]), f
    lo = ref["locOff"]
    for u in range(len(b["reads"])):
        assert rec[u]["editDistance"] == ref["editDistance"][u], u
        assert list(rec[u]["endLocations"] or []) == list(ref["ends"][lo[u]:lo[u + 1]]), u
    assert st["word_steps"] < eligible, st


@pytest.mark.parametrize("name", ["three", "two", "lowcomplexity"])
def test_small_alphabets_and_low_complexity(name, tmp_path):
    """a three-symbol target with reads holding the fourth base; a two-symbol target (buckets around the cap of 64); a
    homopolymer run and a tandem repeat: parity, and the hand-back count against the model"""
    b, ref, st, log = _child(name, tmp_path)
    assert len(set(b["target"].tolist())) == {"three": 3, "two": 2, "lowcomplexity": 4}[name]
    assert _handed_back(b, log)
    (nwd, (K, back, slots)), = log["seed"].items()
    if name != "three":
        assert 0 < back < len(b["reads"]), log                 # (both sides of the caps are in the batch)


def test_probed_batch_in_full(tmp_path):
    """16,448 six-word reads with 0 .. 40 edits at k = -1: the probe stays open, the ladder is priced after a seed pass (no
    level at or below k_f), every read is compared"""
    b, ref, st, log = _child("spread", tmp_path)
    T = len(b["target"])
    assert _nslots(len(b["reads"])) >= 16_384
    K = seed_threshold(min(len(r) for r in b["reads"]), T)
    assert log["seed"][6][0] == K >= 8
    assert int(np.sum(ref["editDistance"] > K)) * 10 > len(b["reads"])
    kfirst, levels = log["ladder"][6]
    assert kfirst == K and all(t > K for t in levels), log
    assert log["levels"][6][0] == int(np.sum(ref["editDistance"] > K))
    assert _handed_back(dict(b, K={6: K}), log)
