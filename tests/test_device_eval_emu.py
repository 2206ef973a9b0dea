"""CPU: the checks of tests/device_eval_common.py -- every device model's stamp of one Newton iteration against the mpmath restatement --
on the host emulation of the kernels (tests/emu: pe_front.hpp with a one-thread team), each case a subprocess with PE_HIP_LIB set.  The
emulation runs the same eval_devices / companion_update text through the same schedules' host logic (resident loop, split schedule with
its dynamic_only iterations and the companion fused into the first evaluation); the device's own exp / log / sin / fmod, its fused
multiply-adds and the strided loops over more devices than a launch has threads are what the GPU twin adds."""
import os
import subprocess
import sys

import pytest

from device_eval_common import IDS, SCHEDULES
from parity_common import ROOT, make


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
import device_eval_common as D
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_diode_mosfet_bjt_stamps_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_nonlinear({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_relay_hysteresis_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_relay({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_time_sources_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_sources({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_trapezoidal_companions_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_companions({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0, "EW_GRID": 1}, {"SPLIT": 1, "GRAPH": 1, "EW_GRID": 3}], ids=["resident", "split_ew1", "split_graph_ew3"])
def test_more_devices_than_threads_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_wrap({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_384_and_instance_order_under_host_emulation(emu_lib, knobs):
    run_emu(emu_lib, f"D.check_batch_384({knobs!r}, 'emulation')")


@pytest.mark.parametrize("which", ["formulas", "nonlinear", "relay", "sources", "companions", "wrap"])
def test_float64_oracle_stays_within_the_bound(emu_lib, which):
    run_emu(emu_lib, f"import pe_load; D.check_oracle_within_bound(pe_load.load_oracle(), {which!r})")
