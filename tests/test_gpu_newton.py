"""The Newton acceptance test on the MI355X at its edges (newton_violations of pe_front.hpp inside the resident kernels in both register
budgets, with and without probes; k_m2_finish of the split schedule through its permutation and its atomicOr over the workgroups, with and
without captured graphs; the host loop m2_point and its active mask) against the restatement of tests/newton_common.py over the device's
own iterates: the checks of tests/test_newton_emu.py on the real library, where the strided row loops, the reductions and the device's
arithmetic (a contracted atol + rtol * m included) are.  Every case is a child process of its own under a time limit; once a child has died
of a signal or run out of time nothing more is started on the GPU (the remaining cases fail without running)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
WRAP = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 1, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 3}]
WRAP_IDS = ["resident", "split_ew1", "split_graph_ew1", "split_ew3"]
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import newton_common as N
"""

_gpu_lost = []


def run_gpu(body, timeout=120):
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    try:
        r = subprocess.run([sys.executable, "-c", PRE + body], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _gpu_lost.append("time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    print(r.stdout)
    assert "NEWTON MI355X" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_inclusive_edge_per_row_class(knobs):
    run_gpu(f"N.check_edges({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", WRAP, ids=WRAP_IDS)
def test_every_thread_position_decides(knobs):
    """the wanted rows on every schedule; on the split schedule k_m2_finish takes its rows through col_src, so there one instance per cell
    lets every row -- hence every thread position of every workgroup, whatever the permutation -- decide"""
    run_gpu(f"""
reached, info = N.check_positions({knobs!r}, 'MI355X')
assert info['n_wavefronts'] * 64 <= N.PE_THREADS < info['rows'], info
assert {knobs.get('EW_GRID', 0)} == 0 or info['ew_grid'] == {knobs.get('EW_GRID', 0)}, info
if {knobs['SPLIT']}:
    reached, info = N.check_positions({knobs!r}, 'MI355X every cell', every_cell=True)
    assert len(reached['node']) == N.WRAP_CELLS and len(reached['branch']) == N.WRAP_CELLS
""")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_relative_term(knobs):
    run_gpu(f"N.check_relative({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_mixed_tolerances_on_a_busy_circuit(knobs):
    run_gpu(f"N.check_busy({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_instances_retire_independently(knobs):
    run_gpu(f"N.check_retire({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_instance_order_at_batch_384(knobs):
    run_gpu(f"N.check_batch_384({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_max_newton_edges(knobs):
    run_gpu(f"N.check_cap({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_nan_is_a_violation(knobs):
    run_gpu(f"N.check_nan({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_transient_steps(knobs):
    run_gpu(f"N.check_transient({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_dc_sweep_inherits_the_options(knobs):
    run_gpu(f"N.check_sweep({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_no_false_alarm_of_the_residual_check(knobs):
    run_gpu(f"N.check_no_false_alarm({knobs!r}, 'MI355X')")
