"""Operating point with gmin / source stepping (pe_hip_analyze_op_stepping / pe_hip_get_op_step_state / pe_hip_get_op_step_log,
pe_hip_sweep_operating_point_stepping, include/pe_hip.h) on the CPU: the engine's host logic and the team-generic controller text
(pe_op_step.hpp) through the host emulation library (tests/emu: test infrastructure), one child process per case, on the resident and on
the split schedule.  The bodies are those of tests/test_gpu_op_step.py (tests/op_step_common.py); the reference is the controller restated
in Python over the unchanged oracle.  The hand mutations of DESIGN.md 8 name the case that catches each."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}]
IDS = ["resident", "split"]


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


def run(emu, call, devices=None):
    e = dict(os.environ, PE_HIP_LIB=emu)
    if devices:
        e["PE_EMU_DEVICES"] = str(devices)
    body = "import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\nimport op_step_common as T\nT.%s\n" % (ROOT, ROOT, call)
    r = subprocess.run([sys.executable, "-c", body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout)
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", ["bjt_npn_ce_dc_fail", "bjt_pnp_ce_op_fail", "bjt_amp_trop_fail"])
def test_goldens_that_fail_directly_are_solved(emu, name, knobs):
    """1 + 2: the log against the restated controller, the solution against the oracle's stepped solution"""
    run(emu, f"check_golden({name!r}, {knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_mixed_batch_has_every_outcome(emu, knobs):
    run(emu, f"check_mixed({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_loops_that_wrap(emu, knobs):
    """258 sources, 258 diodes, 774 rows: each beyond the controller's team of 256"""
    run(emu, f"check_wrap({knobs!r}, 258, 3, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_384(emu, knobs):
    run(emu, f"check_wrap({knobs!r}, 8, 384, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_failure_path(emu, knobs):
    run(emu, f"check_failure({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_relay_state_is_part_of_the_shadow(emu, knobs):
    run(emu, f"check_relay({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_switch_is_never_scaled_and_generator_keeps_its_value(emu, knobs):
    run(emu, f"check_switch_generator({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_refusals_and_the_batch_in_which_nothing_fails(emu, knobs):
    run(emu, f"check_refusals({knobs!r}, 'emulation')")
    run(emu, f"check_overlay({knobs!r}, 'emulation')")


def test_sweep_entry_point_over_two_emulated_devices(emu):
    run(emu, "check_sweep('emulation')", devices=2)


def test_cpp_plug_in_api(emu):
    """tests/cpp/op_step_ce.cpp: circult::analyze() fails on the cold common-emitter stage, circult::analyze_op_stepping() reaches
    v(B) = 0.692889 V with every method"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build_emu/op_step_ce")
    out = subprocess.run([os.path.join(cpp, "_build_emu", "op_step_ce")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"op_step_ce exited {out.returncode}: {out.stderr}"


def test_kernel_text_as_host_program(tmp_path):
    """scripts/op_step_kernel_host.cpp: the controller text with a one-thread team over a hand-made view -- three instances in different
    phases, a ragged source list, a non-finite solution behind a status of OK (the one hand mutation no engine run can reach: the solvers
    report such a solution themselves), a log shorter than the levels.  (The sanitizer build named in its header is run by hand.)"""
    exe = str(tmp_path / "op_step_kernel_host")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-I" + os.path.join(ROOT, "phy-engine_amd", "csrc"), os.path.join(ROOT, "scripts", "op_step_kernel_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
