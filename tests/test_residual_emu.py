"""CPU: the checks of tests/residual_common.py -- the residual safety net of the static-pivot LU against a restatement of eta over the
engine's own A, b and x, on solves that really are inaccurate -- on the host emulation of the kernels (tests/emu), each case a subprocess
with PE_HIP_LIB set.  The emulation runs residual_norms and backward_error of pe_front.hpp with a one-thread team, the serial twins of
k_m2_residual, k_m2_refine_apply, k_m2_clear_eta and k_m2_retest, and the same host loop (m2_check_residuals, prepare_inaccurate_retry);
the strided row loops, team_max4, the atomic maxima over the workgroups and the device's own arithmetic are what the GPU twin adds."""
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
import residual_common as R
{body}
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "RESIDUAL emulation" in r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_inclusive_edge_across_magnitudes_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_edges({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", WRAP, ids=WRAP_IDS)
def test_every_reduction_at_every_thread_position_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_positions({knobs!r}, 'emulation')")


@pytest.mark.parametrize("batch", [3, 65, 384])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_refinement_repairs_per_instance_under_host_emulation(emu_lib, knobs, batch):
    run_emu(emu_lib, f"R.check_repair({knobs!r}, {batch}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_newton_retest_after_a_refinement_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_retest({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_transient_steps_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_transient({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_degenerate_norms_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_degenerate({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_failure_stays_clean_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"R.check_failure({knobs!r}, 'emulation')")
