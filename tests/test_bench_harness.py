"""bench.py as a harness: the --gpus contract, the multi-rank path with the ENGINE on every rank, and the
configs 4 / 5 lines with their full-batch parity.  CPU part: argument plumbing and the checker's arithmetic
(the reference pool posing as the engine).  GPU part (-m gpu): real runs, two ranks sharing the one device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=1200):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=e)


def _line(p):
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_gpus_flag_must_match_the_world_size():
    """`--gpus 3` inside a 2-rank launch would report a wrong n_gpus: refused before anything runs"""
    p = _run(["--gpus", "3"], env={"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "2"})
    assert p.returncode != 0 and "refusing" in (p.stderr + p.stdout)


def test_checker_arithmetic(ref):
    """the parity / invariant code of bench.py on results that are right by construction (the reference pool),
    then with one distance and one end location falsified"""
    if ref is None:
        pytest.skip("oracle/_ref did not travel")
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as O
    old = bench.TARGET_LEN
    bench.TARGET_LEN = 60000
    try:
        w = bench.make_workload(2, 1500, 0, 1, False)
        r = O.pool_align(w["qpool"], w["qoff"], w["tpool"], w["toff"], True, "HW", "distance")
        flat = {k: r[k] for k in ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")}
        flat["starts"] = None
        inv = bench.invariants_config2(w, flat)
        assert inv["ed_le_planted_edits"] and inv["ed_le_read_len"] and inv["planted_position_in_end_locations"]
        assert inv["planted_position_reads_checked"] > 1000
        base, par = bench.cpu_baseline_and_parity(w, flat, 1500)
        assert par["checked"] == 1500 and par["bit_exact"] == 1500 and base["kind"] == "reference" and base["value"] > 0
        flat["ends"] = flat["ends"].copy(); flat["ends"][7] += 1
        base, par = bench.cpu_baseline_and_parity(w, flat, 1500)
        assert par["bit_exact"] == 1499
    finally:
        bench.TARGET_LEN = old
    w = bench.make_workload(5, 64, 0, 1, False)
    r = O.pool_align(w["qpool"], w["qoff"], w["tpool"], w["toff"], False, "NW", "path", want_cigar=True)
    flat = {k: r[k] for k in ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "starts", "alnOff", "alignment")}
    base, par = bench.cpu_baseline_and_parity(w, flat, 64)
    assert par["bit_exact"] == 64 and par["cigar_extended_equal"] and par["cigar_standard_equal"] and par["op_bytes_equal"]


def test_dump_outputs_float_types_and_seeded_sample(tmp_path):
    """--dump-outputs writes float32 where every value is exact in it, float64 otherwise; over the size limit, the same
    seeded positions of every large array, with the positions beside it"""
    sys.path.insert(0, ROOT)
    import bench
    small = np.arange(-5, 1000, dtype=np.int32)
    big = np.array([0, 2 ** 24, 3 * 10 ** 9], dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "whole"), {"small": small, "big": big, "empty": np.zeros(0, dtype=np.uint8)})
    a, b = (np.load(str(tmp_path / "whole" / (n + ".npy"))) for n in ("small", "big"))
    assert a.dtype == np.float32 and np.array_equal(a, small)
    assert b.dtype == np.float64 and np.array_equal(b, big)
    assert sorted(os.listdir(str(tmp_path / "whole"))) == ["big.npy", "small.npy"]          # no empty outputs
    long_ = np.arange(100000, dtype=np.int32) * 7
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"long": long_, "short": small}, limit=80000)
    v, i = np.load(str(tmp_path / "s1" / "long.npy")), np.load(str(tmp_path / "s1" / "long.index.npy"))
    assert 0 < len(v) == len(i) < len(long_) and np.array_equal(v, long_[i.astype(np.int64)])
    assert np.array_equal(v, np.load(str(tmp_path / "s2" / "long.npy")))
    assert np.array_equal(np.load(str(tmp_path / "s1" / "short.npy")), small)
    assert sum(os.path.getsize(str(tmp_path / "s1" / f)) for f in os.listdir(str(tmp_path / "s1"))) < 80000 + 4 * 256


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_two_engine_ranks_agree_with_one(tmp_path):
    """bench.py --gpus 2 spawns two ranks itself (torch.distributed.run, gloo, both on device 0 of this 1-GPU box);
    each runs the HIP engine on its shard; the gathered distances equal a one-rank run of the same global batch"""
    one, two = str(tmp_path / "one.npy"), str(tmp_path / "two.npy")
    common = ["--reads", "6000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-e2e", "--strong"]
    a = _line(_run(common + ["--dump", one]))
    b = _line(_run(common + ["--gpus", "2", "--share-gpu", "--dump", two]))
    assert a["n_gpus"] == 1 and b["n_gpus"] == 2 and b["dry_run_shared_gpu"] and len(b["per_rank_ms_per_step"]) == 2
    assert b["scaling"] == "strong" and b["devices_distinct"] == 1
    x, y = np.load(one), np.load(two)
    assert len(x) == 6000 and np.array_equal(x, y)
    # weak scaling: rank r generates its own batch (seed + r); rank 0's half equals the one-rank run of 3000 reads
    c = _line(_run(["--reads", "3000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-e2e", "--gpus", "2",
                    "--share-gpu", "--dump", two]))
    d = _line(_run(["--reads", "3000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-e2e", "--dump", one]))
    assert c["scaling"] == "weak" and c["n_gpus"] == 2 and d["n_gpus"] == 1
    assert np.array_equal(np.load(two)[:3000], np.load(one))


@pytest.mark.gpu
def test_gpus_2_without_a_second_device_fails_loudly():
    import edlib_amd
    if edlib_amd.device_count() >= 2:
        pytest.skip("this box has a second GPU")
    p = _run(["--gpus", "2", "--reads", "2000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-e2e"])
    assert p.returncode != 0 and "only 1 device" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,units", [(2, 4096), (4, 600), (5, 1500)])
def test_config_lines_carry_full_parity(cfg, units):
    out = _line(_run(["--config", str(cfg), "--units", str(units), "--steps", "1", "--warmup", "1", "--parity-sample", str(units), "--full"]))
    assert out["config"]["baseline_config"] == cfg and out["n_gpus"] == 1
    for key in ("roofline", "valu_roofline", "cpu_baseline", "parity_sample"):
        assert key in out
    assert out["parity_sample"]["checked"] == units and out["parity_sample"]["bit_exact"] == units
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] in ("reference", "port")
    if cfg == 5:
        assert out["parity_sample"]["cigar_extended_equal"] and out["parity_sample"]["cigar_standard_equal"]
    if cfg == 2:
        assert all(v is True for k, v in out["invariants"].items() if k != "planted_position_reads_checked")
        assert out["e2e"]["distances_equal_resident"] is True


@pytest.mark.gpu
@pytest.mark.parametrize("strong", [False, True])
def test_eight_ranks_dry_run_on_one_device(strong):
    """the driver's 8-GPU launch shape on a 1-GPU box: eight ranks (torch.distributed.run, gloo, all on device 0), weak
    and strong scaling; every rank reports, host pools are sized from the CPU quota divided by the world size, and the
    run finishes well inside two minutes"""
    import time
    args = ["--reads", "64000" if strong else "8000", "--steps", "2", "--warmup", "1", "--parity-sample", "400", "--no-e2e",
            "--gpus", "8", "--share-gpu", "--full"] + (["--strong"] if strong else [])
    t0 = time.time()
    out = _line(_run(args, timeout=300))
    wall = time.time() - t0
    assert out["n_gpus"] == 8 and out["dry_run_shared_gpu"] and len(out["per_rank_ms_per_step"]) == 8
    assert out["scaling"] == ("strong" if strong else "weak") and out["devices_distinct"] == 1
    assert out["config"]["units_per_gpu"] == 8000
    # a multi-rank line carries its evidence: the reference over a sample of rank 0's shard, after the timed region
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] in ("reference", "port")
    assert out["parity_sample"]["checked"] >= 400 and out["parity_sample"]["bit_exact"] == out["parity_sample"]["checked"]
    assert out["parity_sample"]["shard"] == "rank 0 of 8" and all(v is True for k, v in out["invariants"].items() if k != "planted_position_reads_checked")
    assert wall < 150, wall


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,units", [(2, 4096), (5, 300)])
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, cfg, units):
    """a plain line holds the headline of exactly --steps timed steps and none of --full's extras; --dump-outputs writes
    the results of the last step as floats, the same from run to run"""
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        out = _line(_run(["--config", str(cfg), "--units", str(units), "--steps", "2", "--warmup", "1", "--dump-outputs", d,
                          "--dump", str(tmp_path / "ed.npy")]))
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "GCUPS" and out["higher_is_better"] is True and out["dtype"] == "u32"
        for key in ("cpu_baseline", "parity_sample", "e2e", "secondary", "clocks"):
            assert key not in out
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert all(n + ".npy" in names for n in ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends"))
    if cfg == 5:
        assert all(n + ".npy" in names for n in ("starts", "alnOff", "alignment", "cigar_extended_chars", "cigar_standard_off"))
    else:                                       # TASK_DISTANCE: no op bytes, so no path arrays
        assert "alignment.npy" not in names and "alnOff.npy" not in names
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.array_equal(a, b), n
    ed = np.load(os.path.join(dirs[0], "editDistance.npy"))
    assert len(ed) == units and np.array_equal(ed, np.load(str(tmp_path / "ed.npy")))
