"""The window check of the stored-result getters at its edges, and what makes a stored result unreadable (tests/result_windows_common.py),
on the CPU: the engine's host logic through the host emulation library (tests/emu: test infrastructure), one child process per case."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


PRE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import pe_load
pe = pe_load.load()
import result_windows_common as RW
''' % (ROOT, ROOT)


def run(emu, body):
    r = subprocess.run([sys.executable, "-c", PRE + body], env=dict(os.environ, PE_HIP_LIB=emu), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-3000:])


def test_windows(emu):
    """every getter, every combination of the nine (first, n) and the nine (first_instance, count) pairs, sentinel-filled buffers"""
    run(emu, "RW.check_windows(pe)\n")


def test_validity(emu):
    """pe_hip_update_param and pe_hip_set_dc_sweep_rows: every getter answers with its own "no ... yet" """
    run(emu, "RW.check_validity(pe)\n")
