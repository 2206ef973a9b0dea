"""CPU: the checks of tests/ac_stamp_common.py -- every device's small-signal stamp, the sweep's device-side fill, the adjoint system and
the solve chain against the mpmath restatement -- on the host emulation of the kernels (tests/emu), each case a subprocess with PE_HIP_LIB
set.  The emulation runs build_ac_circuit / fill_ac_values (host code in the product too) and the text of ac_sweep_fill, ac_residual and
ac_residual_each with a one-thread team; the grid-strided loops over more slots than a workgroup has threads, the wave reductions of the
backward error and the device's own arithmetic are what the GPU twin adds."""
import os
import subprocess
import sys

import pytest

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
import ac_stamp_common as A
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


@pytest.mark.parametrize("g_min", [0.0, 2.0 ** -40], ids=["gmin0", "gmin"])
def test_one_device_per_deck_under_host_emulation(emu_lib, g_min):
    run_emu(emu_lib, f"A.check_single({{}}, 'emulation', {g_min!r})")


def test_infinite_inductor_at_omega_zero_under_host_emulation(emu_lib):
    run_emu(emu_lib, "A.check_inf_inductor({}, 'emulation')")


@pytest.mark.parametrize("big", [False, True], ids=["one_block", "five_blocks"])
@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}], ids=["resident", "split"])
def test_mixed_deck_under_host_emulation(emu_lib, knobs, big):
    run_emu(emu_lib, f"A.check_mixed({knobs!r}, 'emulation', big={big!r})")


def test_adjoint_system_under_host_emulation(emu_lib):
    run_emu(emu_lib, "A.check_adjoint({}, 'emulation')")


def test_nan_instance_under_host_emulation(emu_lib):
    run_emu(emu_lib, "A.check_nan_instance({}, 'emulation')")


def test_band_edge_under_host_emulation(emu_lib):
    run_emu(emu_lib, "A.check_band_edge({}, 'emulation')")


@pytest.mark.parametrize("which", ["single", "single_gmin", "mixed"])
def test_float64_oracle_stays_within_the_bound(emu_lib, which):
    run_emu(emu_lib, f"import pe_load; A.check_oracle_within_bound(pe_load.load_oracle(), {which!r})")
