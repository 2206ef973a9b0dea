"""CPU: the checks of tests/test_gpu_front_shapes.py on the host emulation of the kernels (tests/emu: pe_front.hpp / pe_quad.hpp lane by
lane, one-thread team), each in a subprocess with PE_HIP_LIB set.  They pin the class tables -- which fronts the gadget circuits of
tests/front_shapes_common.py put ON the limits of the front classes is host logic and the same on the device -- and the isolation of a
bad instance, and show that the inputs are healthy with the reference alone.  The device-only parts (DPP row broadcasts, the register
image, the LDS layouts) are what the GPU twin adds."""
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
import numpy as np
import front_shapes_common as F
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 7])
def test_parity_per_instance_under_host_emulation(emu_lib, batch):
    run_emu(emu_lib, f"F.check_parity(F.new_engine(), {batch})")


def test_many_children_under_host_emulation(emu_lib):
    run_emu(emu_lib, "F.check_parity(F.new_engine(F.KNOBS_MANY_CHILDREN), 3, F.DEFAULT_CLASSES + F.KNOB_CLASSES, 'many children')")


def test_slot_independence_under_host_emulation(emu_lib):
    run_emu(emu_lib, "F.check_slot_independence(F.new_engine())")


def test_one_bad_instance_in_a_quad_under_host_emulation(emu_lib):
    run_emu(emu_lib, "F.check_one_bad_instance(F.new_engine())")


@pytest.mark.parametrize("name", ["chain200", "chain100"])
def test_real_seam_patterns_under_host_emulation(emu_lib, name):
    run_emu(emu_lib, f"F.check_real_seam(F.pe.ffi.Engine(), {name!r})")


def test_complex_seam_pattern_under_host_emulation(emu_lib):
    run_emu(emu_lib, "F.check_complex_seam(F.pe.ffi.Engine(), 'chain100')")
