"""CPU: the checks of tests/newton_common.py -- the Newton acceptance test at its edges, against a restatement in plain double over the
engine's own iterates -- on the host emulation of the kernels (tests/emu), each case a subprocess with PE_HIP_LIB set.  The emulation runs
newton_violations of pe_front.hpp with a one-thread team and the serial twin of k_m2_finish through the same host logic (m2_point and its
active mask, the options, checkpoints, probes, the sweep engine); the strided row loops, the reductions over wavefronts and workgroups
and the device's own arithmetic are what the GPU twin adds."""
import os
import subprocess
import sys

import pytest

from device_eval_common import IDS, SCHEDULES
from parity_common import ROOT, make

WRAP = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 1, "EW_GRID": 3}]
WRAP_IDS = ["resident", "split_ew1", "split_graph_ew3"]


@pytest.fixture(scope="module")
def emu_lib():
    emu = os.path.join(ROOT, "tests", "emu")
    make("-C", emu)
    return os.path.join(emu, "libpe_hip_emu.so")


def run_emu(emu_lib, body):
    code = f"""
import os, sys
os.environ['PE_HIP_LIB'] = {emu_lib!r}
sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import newton_common as N
{body}
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "NEWTON emulation" in r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_inclusive_edge_per_row_class_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_edges({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", WRAP, ids=WRAP_IDS)
def test_every_thread_position_decides_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_positions({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_relative_term_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_relative({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_mixed_tolerances_on_a_busy_circuit_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_busy({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_instances_retire_independently_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_retire({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_instance_order_at_batch_384_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_batch_384({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_max_newton_edges_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_cap({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_nan_is_a_violation_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_nan({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_transient_steps_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_transient({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_dc_sweep_inherits_the_options_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_sweep({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_no_false_alarm_of_the_residual_check_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"N.check_no_false_alarm({knobs!r}, 'emulation')")
