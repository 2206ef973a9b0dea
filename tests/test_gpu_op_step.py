"""GPU (MI355X): operating point with gmin / source stepping (pe_hip_analyze_op_stepping, include/pe_hip.h) -- k_op_step_control of
pe_kernels.hip between the engine's own solves, on the resident and on the split schedule.  The bodies are shared with the host emulation
(tests/op_step_common.py, tests/test_op_step_emu.py); the reference is the controller restated in Python over the unchanged oracle.  What
the device adds: the 256-thread workgroup per instance, its ballot + LDS finiteness flag, the strided copies to and from the shadow and the
source-slot loop beyond one team (258 cells), the libm call behind the gmin values.  Every case is a child process of its own under a time
limit; once a child has died of a signal or run out of time nothing more is started on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import op_step_common as T
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
    assert "OPSTEP MI355X" in r.stdout
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
@pytest.mark.parametrize("name", ["bjt_npn_ce_dc_fail", "bjt_pnp_ce_op_fail", "bjt_amp_trop_fail"])
def test_goldens_that_fail_directly_are_solved(name, knobs):
    run_gpu(f"check_golden({name!r}, {knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_mixed_batch_has_every_outcome(knobs):
    run_gpu(f"check_mixed({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_loops_that_wrap(knobs):
    """258 sources, 258 diodes, 774 rows: each beyond the controller's workgroup of 256"""
    run_gpu(f"check_wrap({knobs!r}, 258, 3, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_batch_384(knobs):
    """the resident kernels' 128-VGPR build; 384 workgroups of the controller"""
    run_gpu(f"check_wrap({knobs!r}, 8, 384, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_failure_path(knobs):
    run_gpu(f"check_failure({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_relay_state_is_part_of_the_shadow(knobs):
    run_gpu(f"check_relay({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_switch_is_never_scaled_and_generator_keeps_its_value(knobs):
    run_gpu(f"check_switch_generator({knobs!r}, 'MI355X')")


def test_refusals_and_the_batch_in_which_nothing_fails():
    run_gpu("check_refusals({'SPLIT': 0}, 'MI355X'); print('OPSTEP MI355X refusals')")
    run_gpu("check_overlay({'SPLIT': 1, 'GRAPH': 0}, 'MI355X'); print('OPSTEP MI355X overlay')")


def test_cpp_plug_in_api():
    """tests/cpp/op_step_ce.cpp against the product library: circult::analyze() fails on the cold common-emitter stage,
    circult::analyze_op_stepping() reaches v(B) = 0.692889 V with every method"""
    from parity_common import make
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build/op_step_ce")
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    out = subprocess.run([os.path.join(cpp, "_build", "op_step_ce")], capture_output=True, text=True, timeout=120)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {out.returncode}")
    assert out.returncode == 0, f"op_step_ce exited {out.returncode}: {out.stderr}"
