"""DC sweep with the points as batched instances (pe_hip_set_dc_sweep_rows / pe_hip_analyze_dc_sweep / pe_hip_get_dc_sweep / _status,
include/pe_hip.h) on the CPU: the engine's host logic and the team-generic kernel text (pe_dc_sweep.hpp) through the host emulation
library (tests/emu: test infrastructure), one child process per case.  The bodies are those of tests/test_gpu_dc_sweep.py
(tests/dc_sweep_common.py); what the device adds to them are the wavefront scans of the classification."""
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


def run(emu, call):
    e = dict(os.environ, PE_HIP_LIB=emu)
    e.pop("PHY_ENGINE_HIP_DC_SWEEP_POINTS", None)
    body = "import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\nimport dc_sweep_common as T\nT.%s\n" % (ROOT, ROOT, call)
    r = subprocess.run([sys.executable, "-c", body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_linear_sweeps_against_the_oracle(emu):
    run(emu, "check_linear()")


@pytest.mark.parametrize("name", ["diode_op", "nmos", "mesh"])
def test_nonlinear_without_continuation(emu, name):
    run(emu, "check_nonlinear_no_continuation(%r)" % name)


def test_instance_and_point_mapping(emu):
    run(emu, "check_mapping()")


def test_continuation_converges_the_diode_chain(emu):
    run(emu, "check_continuation()")


def test_continuation_stops_without_progress(emu):
    run(emu, "check_no_progress()")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_classification_at_its_edges(emu, n):
    run(emu, "check_classify_edges(%d)" % n)


def test_trace_order(emu):
    run(emu, "check_trace()")


def test_isolation_and_refusals(emu):
    run(emu, "check_isolation_and_refusals()")
    run(emu, "check_overlay_refused()")
