"""GPU (MI355X): DC sweep with the points as batched instances (pe_hip_analyze_dc_sweep, include/pe_hip.h) -- k_dc_sweep_fill / _seed /
_classify / _gather of pe_kernels.hip around the engine's own solves.  The bodies are shared with the host emulation
(tests/dc_sweep_common.py, tests/test_dc_sweep_emu.py); references are the oracle and the main engine's single-point path."""
import pytest

import dc_sweep_common as T

pytestmark = pytest.mark.gpu


def test_linear_sweeps_against_the_oracle():
    T.check_linear()


@pytest.mark.parametrize("name", ["diode_op", "nmos", "mesh"])
def test_nonlinear_without_continuation(name):
    T.check_nonlinear_no_continuation(name)


def test_instance_and_point_mapping():
    T.check_mapping()


def test_continuation_converges_the_diode_chain():
    T.check_continuation()


def test_continuation_stops_without_progress():
    T.check_no_progress()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_classification_at_its_edges(n):
    """one pass of n slots: fewer than a wavefront, one exactly, one more, more than a workgroup's chunk of 256"""
    T.check_classify_edges(n)


def test_trace_order():
    T.check_trace()


def test_isolation_and_refusals():
    T.check_isolation_and_refusals()
    T.check_overlay_refused()
