"""Backward-Euler and Gear-2 integration of the transient (pe_hip_set_tr_method / pe_hip_get_tr_history / pe_hip_sweep_set_tr_method,
include/pe_hip.h) on the CPU: the engine's host logic and the team-generic device text (pe_integ.hpp) through the host emulation library
(tests/emu: test infrastructure), one child process per case, on the three schedules.  The bodies are those of tests/test_gpu_integ.py
(tests/integ_common.py); the reference is the dense descriptor-form integrator restated there."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
DECKS = ["c_only", "l_only", "kl_only", "d_only", "mixed"]


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


def run(emu, call):
    e = dict(os.environ, PE_HIP_LIB=emu)
    body = "import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\nimport integ_common as T\nT.%s\n" % (ROOT, ROOT, call)
    r = subprocess.run([sys.executable, "-c", body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout)
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", DECKS)
def test_every_device_kind_and_offset_of_the_packed_history(emu, name, knobs):
    """1: decks with one kind only and one with all four, BE and GEAR2, batch 1, 3 and 65"""
    run(emu, "; T.".join(f"check_devices({name!r}, {m}, {b}, {knobs!r}, 'emulation')" for m in (1, 2) for b in (1, 3, 65)))


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_variable_ratios_and_the_fallback_at_ratio_3(emu, knobs):
    run(emu, f"check_ratios({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_factor_reuse_of_a_linear_circuit_is_keyed_on_a0(emu, knobs):
    run(emu, f"check_factor_reuse({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_l_stability(emu, knobs):
    """3: the reason for the feature -- the trapezoidal inductor voltage alternates for ten steps, BE and GEAR2 are gone after six"""
    run(emu, f"check_l_stability({knobs!r}, 'emulation')")


def test_the_restatement_alone_is_inside_every_order_bracket():
    from integ_common import check_order_restatement
    check_order_restatement()


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_order(emu, knobs):
    run(emu, f"check_order({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_history_across_launches_and_checkpoints(emu, knobs):
    run(emu, f"check_launches({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_restart_rules(emu, knobs):
    run(emu, f"check_restarts({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_default_untouched(emu, knobs):
    run(emu, f"check_default({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("method", [1, 2], ids=["be", "gear2"])
def test_pinned_controller_equals_fixed_step_bitwise(emu, method, knobs):
    run(emu, f"check_controller_pinned({method}, {knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("method", [1, 2], ids=["be", "gear2"])
def test_replay_reproduces_every_accepted_point_and_decision(emu, method, knobs):
    run(emu, f"check_controller_replay({method}, {knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_first_step_after_a_source_breakpoint_is_a_be_step(emu, knobs):
    run(emu, f"check_controller_breakpoint({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("method", [1, 2], ids=["be", "gear2"])
def test_a_nan_in_the_history_is_never_accepted(emu, method, knobs):
    run(emu, f"check_controller_nan({method}, {knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_refusals(emu, knobs):
    run(emu, f"check_refusals({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_sweep_twin(emu, knobs):
    run(emu, f"check_sweep({knobs!r}, 'emulation')")


def test_cpp_plug_in_api(emu):
    """tests/cpp/integ_ringing.cpp: the three assertions of the L-stability case through circult::set_tr_method"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build_emu/integ_ringing")
    r = subprocess.run([os.path.join(cpp, "_build_emu", "integ_ringing")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"integ_ringing exited {r.returncode}: {r.stdout} {r.stderr}"


def test_kernel_text_as_host_program(tmp_path):
    """scripts/integ_kernel_host.cpp: the text of pe_integ.hpp with a one-thread team over a hand-made view whose buffers have exactly the
    engine's sizes.  (The sanitizer build named in its header is run by hand.)"""
    exe = str(tmp_path / "integ_kernel_host")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-I" + os.path.join(ROOT, "phy-engine_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "integ_kernel_host.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
