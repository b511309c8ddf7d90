"""-m gpu: the pairs of flat_cigar_cases.py (runs that end on op 63, 64 and 65, runs across trips, 64 closes in one trip,
a class change at a trip edge under one M, run lengths at every digit count -- test_flat_cigar_cases.py shows on the
reference's strings that they get there) through flat pair batches: every field and both CIGAR forms of every unit
against the reference."""
import pytest

import flat_cigar_cases as cases
from test_gpu_flat_pairs import _check_task, _flat_launches

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [-1, 8])           # 8: the gap blocks and most mutated pairs have no alignment, an empty string
def test_nw_cigar_edges(engine, k):
    qs, ts, what = cases.nw_pairs()
    st = _check_task(engine, qs, ts, "NW", "path", k=k, what="cigar edges")
    assert st["scan_launches"] == _flat_launches("NW", "path"), st      # the run stayed flat: the strings were the device's


@pytest.mark.parametrize("mode", ["HW", "SHW"])
def test_lead_insert_cigars_beside_window_pairs(engine, mode):
    qs, ts, what = cases.window_pairs()
    st = _check_task(engine, qs, ts, mode, "path", what="lead inserts")
    assert st["scan_launches"] == _flat_launches(mode, "path") and st["overflow_units"] == 0, st
