"""Fourier analysis of transient probes (pe_hip_set_fourier / pe_hip_get_fourier, pe_hip_sweep_set_fourier / _get_fourier,
include/pe_hip.h) on the CPU: the engine's host logic and the team-generic kernel text (pe_fourier.hpp) through the host emulation
library (tests/emu: test infrastructure), one child process per case, on the resident and on the split schedule.  The bodies are those of
tests/test_gpu_fourier.py (tests/fourier_common.py); the reference is the exact integral restated in mpmath over the engine's own accepted
points, and closed forms that do not depend on the steps.  The hand mutations of DESIGN.md name the case that catches each."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
DECKS = ["pulse_src", "vac_r", "rectifier", "pulse_rc"]


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


def run(emu, call, devices=None):
    e = dict(os.environ, PE_HIP_LIB=emu)
    if devices:
        e["PE_EMU_DEVICES"] = str(devices)
    body = "import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\nimport fourier_common as T\nT.%s\n" % (ROOT, ROOT, call)
    r = subprocess.run([sys.executable, "-c", body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout)
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", DECKS)
def test_restatement_fixed_steps(emu, name, knobs):
    """check 1: H = 63 with one probe is exactly one wavefront of work items (vac_r needs it: its first alias is k = 63)"""
    run(emu, f"check_restatement({name!r}, {knobs!r}, 'emulation', H=63)")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
@pytest.mark.parametrize("name", DECKS)
def test_restatement_adaptive(emu, name, knobs):
    run(emu, f"check_restatement({name!r}, {knobs!r}, 'emulation', H=63, adaptive=True)")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_work_items_two_and_576_with_duplicates(emu, knobs):
    """H = 1 with one probe: 2 items (no harmonic k >= 2 exists, so check_instance runs without the signal condition there);
    H = 63 with 9 probes: 576 items wrap the 64-thread and the 512-thread team; duplicates are bit-equal"""
    run(emu, f"check_restatement('rectifier', {knobs!r}, 'emulation', H=63, probes=(0, 1, 0, 2, 1, 0, 2, 2, 0))")
    run(emu, f"check_two_items({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
@pytest.mark.parametrize("name", ["rectifier", "pulse_src"])
def test_restatement_batch_3(emu, name, knobs):
    run(emu, f"check_restatement({name!r}, {knobs!r}, 'emulation', H=9, probes=(0, 1), batch=3)")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_batch_384(emu, knobs):
    run(emu, f"check_batch_384({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_closed_form_trapezoid(emu, knobs):
    run(emu, f"check_closed_pulse({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_closed_form_sampled_sine(emu, knobs):
    run(emu, f"check_closed_sine({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_sample_buffer_does_not_reach_the_accumulation(emu, knobs):
    run(emu, f"check_sample_buffer({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_instances_equal_their_single_runs(emu, knobs):
    run(emu, f"check_batch({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_window_rules(emu, knobs):
    run(emu, f"check_window_rules({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_adaptive_rejected_steps_record_nothing(emu, knobs):
    run(emu, f"check_adaptive_rejections({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_series_arm_at_tiny_steps(emu, knobs):
    run(emu, f"check_tiny_steps({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_compensated_sum_long_run(emu, knobs):
    run(emu, f"check_compensation({knobs!r}, 'emulation')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_refusals(emu, knobs):
    run(emu, f"check_refusals({knobs!r}, 'emulation')")


def test_sweep_handle_over_two_emulated_devices(emu):
    run(emu, "check_sweep('emulation')", devices=2)


def test_cpp_plug_in_api(emu):
    """tests/cpp/fourier_rectifier.cpp through circult: THD of the rectifier against the value the Python reference gives for the same run,
    within the propagated bound, and the harmonics of pulse_src against the closed form"""
    out = run(emu, "__name__; print('EXPECT %.17g %.17g' % T.cpp_expectations({'SPLIT': 0}, 'emulation'))")
    thd, bound = next(line.split()[1:3] for line in out.splitlines() if line.startswith("EXPECT"))
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build_emu/fourier_rectifier")
    r = subprocess.run([os.path.join(cpp, "_build_emu", "fourier_rectifier"), thd, bound], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"fourier_rectifier exited {r.returncode}: {r.stdout} {r.stderr}"


def test_kernel_text_as_host_program(tmp_path):
    """scripts/fourier_kernel_host.cpp: the kernel text with a one-thread team over a hand-made view whose buffers have exactly the
    engine's sizes.  (The sanitizer build named in its header is run by hand.)"""
    exe = str(tmp_path / "fourier_kernel_host")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-I" + os.path.join(ROOT, "phy-engine_amd", "csrc"), os.path.join(ROOT, "scripts", "fourier_kernel_host.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
