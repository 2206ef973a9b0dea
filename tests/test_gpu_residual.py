"""The residual safety net of the static-pivot LU on the MI355X (residual_norms and backward_error of pe_front.hpp inside the resident
kernels in both register budgets, reduced by team_max4; k_m2_residual with its atomic maxima over the workgroups, k_m2_refine_apply through
col_src, k_m2_clear_eta, k_m2_retest and launch_m2_refine of the split schedule, with and without captured graphs; the host loop
m2_check_residuals and the retries of prepare_inaccurate_retry) against the restatement of tests/residual_common.py over the device's own
A, b and x: the checks of tests/test_residual_emu.py on the real library, where the strided row loops, the reductions and the device's
arithmetic (contracted multiply-adds included) are.  Every case is a child process of its own under a time limit; once a child has died
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
import residual_common as R
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
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "RESIDUAL MI355X" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_inclusive_edge_across_magnitudes(knobs):
    run_gpu(f"R.check_edges({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", WRAP, ids=WRAP_IDS)
def test_every_reduction_at_every_thread_position(knobs):
    run_gpu(f"""
name, info = R.check_positions({knobs!r}, 'MI355X')
assert info['n_wavefronts'] * 64 <= R.PE_THREADS < info['rows'], info
assert {knobs.get('EW_GRID', 0)} == 0 or info['ew_grid'] == {knobs.get('EW_GRID', 0)}, info
""")


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [3, 65, 384])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_refinement_repairs_per_instance(knobs, batch):
    run_gpu(f"R.check_repair({knobs!r}, {batch}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_newton_retest_after_a_refinement(knobs):
    run_gpu(f"R.check_retest({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_transient_steps(knobs):
    run_gpu(f"R.check_transient({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_degenerate_norms(knobs):
    run_gpu(f"R.check_degenerate({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_failure_stays_clean(knobs):
    run_gpu(f"R.check_failure({knobs!r}, 'MI355X')")
