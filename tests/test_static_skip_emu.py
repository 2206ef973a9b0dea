"""CPU: the checks of tests/test_gpu_static_skip.py on the host emulation of the kernels (tests/emu), each in a subprocess with PE_HIP_LIB
set.  The classification, the second quad program, the persistent slots of the static roots, the kept forward-substituted pivots and the
host's rule for when to skip are host logic and index data: the emulation walks the same tables lane by lane.  What the GPU twin adds is the
kernels reading them on the device and the captured launch sequences."""
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


def run_emu(emu_lib, body, env=None):
    code = f"""
import os, sys
os.environ['PE_HIP_LIB'] = {emu_lib!r}
sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import static_skip_common as S
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_bit_identity_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_bit_identity()")


def test_bit_identity_many_children_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_bit_identity(S.KNOBS_MANY_CHILDREN, 'many children')")


def test_bit_identity_captured_sequences_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_bit_identity({'GRAPH': 1}, 'captured sequences')")


def test_classification_reaches_every_case_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_classification()")


def test_instances_leaving_mid_point_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_leaving()")


def test_refinement_ends_the_skip_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_refinement()")


def test_fallbacks_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_linear(); S.check_overlay()")


def test_full_stamp_fallback_under_host_emulation(emu_lib):
    run_emu(emu_lib, "S.check_full_stamp()", {"PHY_ENGINE_HIP_FULL_STAMP": "1"})
