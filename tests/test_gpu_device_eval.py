"""Every device model's stamp of one Newton iteration on the MI355X (eval_devices / companion_update of pe_front.hpp inside the resident
kernels in both register budgets and inside k_m2_eval of the split schedule, with and without captured graphs) against the mpmath
restatement of tests/device_eval_common.py: the checks of tests/test_device_eval_emu.py on the real library, where the device's own
exp / log / sin / fmod, its fused multiply-adds and the strided device loops are.  Every case is a child process of its own under a time
limit; once a child has died of a signal or run out of time nothing more is started on the GPU (the remaining cases fail without running)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import device_eval_common as D
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
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_diode_mosfet_bjt_stamps(knobs):
    assert "RATIOS" in run_gpu(f"D.check_nonlinear({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_relay_hysteresis(knobs):
    assert "RATIOS" in run_gpu(f"D.check_relay({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_time_sources(knobs):
    assert "RATIOS" in run_gpu(f"D.check_sources({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_trapezoidal_companions(knobs):
    assert "RATIOS" in run_gpu(f"D.check_companions({knobs!r}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 1, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 3}],
                         ids=["resident", "split_ew1", "split_graph_ew1", "split_ew3"])
def test_more_devices_than_threads(knobs):
    """WRAP_CELLS cells of each kind: the loops of the resident kernel and of k_m2_eval at one workgroup wrap"""
    assert "RATIOS" in run_gpu(f"""
W, info = D.check_wrap({knobs!r}, 'MI355X')
assert info['n_wavefronts'] * 64 <= D.PE_THREADS < D.WRAP_CELLS and D.M2_EVAL_THREADS < D.WRAP_CELLS, info
assert {knobs.get('EW_GRID', 0)} == 0 or info['ew_grid'] == {knobs.get('EW_GRID', 0)}, info
""")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_384_and_instance_order(knobs):
    assert "RATIOS" in run_gpu(f"D.check_batch_384({knobs!r}, 'MI355X')")
