"""CPU: the checks of tests/test_gpu_branch_grid.py on the host emulation of the kernels (tests/emu), each in a subprocess with PE_HIP_LIB
set.  The circuits of tests/branch_grid_common.py -- a third of the rows branch rows, an unsymmetric pattern, a row matching that moves
most of the rows -- are where the static choice of pivots decides the accuracy, and that choice (pe_symbolic.cpp match_rows) is host code
and the same on the device: a matching that strings small pivots together fails here as it does there.  So do the residual checks of the
two solver seams, which are host logic around two small kernels."""
import os
import subprocess
import sys

import pytest

from parity_common import ROOT, make
import branch_grid_common as G


@pytest.fixture(scope="module")
def emu_lib():
    emu = os.path.join(ROOT, "tests", "emu")
    make("-C", emu)
    return os.path.join(emu, "libpe_hip_emu.so")


def run_emu(emu_lib, body):
    code = f"""
import os, sys
os.environ['PE_HIP_LIB'] = {emu_lib!r}
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import pe_load
import branch_grid_common as G
O = pe_load.load_oracle()
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


@pytest.mark.parametrize("knobs", G.SCHEDULES_24, ids=G.IDS_24)
@pytest.mark.parametrize("seed", G.SEEDS[24])
def test_dc_first_step_and_four_steps_24_under_host_emulation(emu_lib, seed, knobs):
    run_emu(emu_lib, f"G.check_all({knobs!r}, 24, {seed}, O, 'emulation')")


@pytest.mark.parametrize("knobs", G.VARIANTS_44, ids=G.IDS_44)
@pytest.mark.parametrize("seed", G.SEEDS[44])
def test_dc_first_step_and_four_steps_44_under_host_emulation(emu_lib, seed, knobs):
    run_emu(emu_lib, f"G.check_all({knobs!r}, 44, {seed}, O, 'emulation')")


@pytest.mark.parametrize("seed", G.SEEDS[44])
def test_static_skip_is_bit_identical_44_under_host_emulation(emu_lib, seed):
    run_emu(emu_lib, f"G.check_static_skip(44, {seed}, O, 'emulation')")


@pytest.mark.parametrize("W,seed", [(W, s) for W in G.SEEDS for s in G.SEEDS[W]])
def test_solver_seams_under_host_emulation(emu_lib, W, seed):
    run_emu(emu_lib, f"G.check_seams({W}, {seed}, 'emulation')")


@pytest.mark.parametrize("name", G.AC_GOLDENS)
def test_ac_stamps_through_the_complex_seam_under_host_emulation(emu_lib, name):
    run_emu(emu_lib, f"G.check_ac_stamps({name!r}, O, 'emulation')")
