"""GPU (MI355X): backward-Euler and Gear-2 integration of the transient (pe_hip_set_tr_method / pe_hip_get_tr_history /
pe_hip_sweep_set_tr_method, include/pe_hip.h) -- integ_step_update inside k_tr_steps_integ on the resident schedule (the barrier between
the reads of h_p and its commit in a 512-thread team), k_m2_integ_update + k_m2_integ_commit in front of the evaluation launch on the split
schedule, with and without captured graphs, k_integ_restart and k_tr_lte_integ.  The bodies are shared with the host emulation
(tests/integ_common.py, tests/test_integ_emu.py); the reference is the dense descriptor-form integrator restated there.  Every case is a
child process of its own under a time limit; once a child has died of a signal or run out of time nothing more is started on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
DECKS = ["c_only", "l_only", "kl_only", "d_only", "mixed"]
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import integ_common as T
"""
_gpu_lost = []


def run_gpu(body, timeout=120):
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    try:
        r = subprocess.run([sys.executable, "-c", PRE + "T." + body], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _gpu_lost.append("time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    print(r.stdout)
    assert "MI355X" in r.stdout
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", DECKS)
def test_every_device_kind_and_offset_of_the_packed_history(name, knobs):
    """1: decks with one kind only and one with all four, BE and GEAR2, batch 1, 3 and 65"""
    run_gpu("; T.".join(f"check_devices({name!r}, {m}, {b}, {knobs!r}, 'MI355X')" for m in (1, 2) for b in (1, 3, 65)))


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_variable_ratios_and_l_stability(knobs):
    """2 and 3"""
    run_gpu(f"check_ratios({knobs!r}, 'MI355X'); T.check_l_stability({knobs!r}, 'MI355X'); T.check_factor_reuse({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_order(knobs):
    """4 (the reference value is the restatement's, computed once per child on the CPU)"""
    run_gpu(f"check_order({knobs!r}, 'MI355X')", timeout=300)


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_history_across_launches_and_restart_rules(knobs):
    """5 and 6"""
    run_gpu(f"check_launches({knobs!r}, 'MI355X'); T.check_restarts({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_default_untouched(knobs):
    run_gpu(f"check_default({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_controller(knobs):
    """8: pinned, replay with re-derived decisions, breakpoint, NaN"""
    run_gpu("; T.".join([f"check_controller_pinned({m}, {knobs!r}, 'MI355X')" for m in (1, 2)] + [f"check_controller_replay({m}, {knobs!r}, 'MI355X')" for m in (1, 2)] +
                        [f"check_controller_breakpoint({knobs!r}, 'MI355X')"] + [f"check_controller_nan({m}, {knobs!r}, 'MI355X')" for m in (1, 2)]), timeout=300)


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_refusals_and_sweep_twin(knobs):
    """9 and 10"""
    run_gpu(f"check_refusals({knobs!r}, 'MI355X'); T.check_sweep({knobs!r}, 'MI355X')")


def test_cpp_plug_in_api():
    """tests/cpp/integ_ringing.cpp against the product library"""
    from parity_common import make
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build/integ_ringing")
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    r = subprocess.run([os.path.join(cpp, "_build", "integ_ringing")], capture_output=True, text=True, timeout=120)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, f"integ_ringing exited {r.returncode}: {r.stdout} {r.stderr}"
