"""GPU (MI355X): Fourier analysis of transient probes (pe_hip_set_fourier / pe_hip_get_fourier, include/pe_hip.h) -- fourier_record inside
k_tr_steps<MINW, true> on the resident schedule and inside k_probe_record on the split schedule, with and without captured graphs, and
k_fourier_finish.  The bodies are shared with the host emulation (tests/fourier_common.py, tests/test_fourier_emu.py); the reference is the
exact integral restated in mpmath over the engine's own accepted points, with a running rounding bound, and closed forms.  What the device
adds: work items spread over 64 and 512 lanes (2, 64 and 576 items), the phasor kept per lane, the device's sincos, the 128-VGPR resident
build at batch 384.  Every case is a child process of its own under a time limit; once a child has died of a signal or run out of time
nothing more is started on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]
DECKS = ["pulse_src", "vac_r", "rectifier", "pulse_rc"]
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import fourier_common as T
"""
_gpu_lost = []


def run_gpu(body, timeout=120):
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    try:
        r = subprocess.run([sys.executable, "-c", PRE + "T." + body], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _gpu_lost.append("time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    print(r.stdout)
    assert "MI355X" in r.stdout
    return r.stdout


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", DECKS)
def test_restatement_fixed_steps(name, knobs):
    """check 1: H = 63 with one probe is exactly one wavefront of work items"""
    run_gpu(f"check_restatement({name!r}, {knobs!r}, 'MI355X', H=63)")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
@pytest.mark.parametrize("name", DECKS)
def test_restatement_adaptive(name, knobs):
    run_gpu(f"check_restatement({name!r}, {knobs!r}, 'MI355X', H=63, adaptive=True)")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_work_items_two_and_576_with_duplicates(knobs):
    """2 items; 576 items wrap the 64-lane workgroup of k_probe_record and the 512-thread workgroup of the resident kernel"""
    run_gpu(f"check_restatement('rectifier', {knobs!r}, 'MI355X', H=63, probes=(0, 1, 0, 2, 1, 0, 2, 2, 0)); T.check_two_items({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
@pytest.mark.parametrize("name", ["rectifier", "pulse_src"])
def test_restatement_batch_3(name, knobs):
    run_gpu(f"check_restatement({name!r}, {knobs!r}, 'MI355X', H=9, probes=(0, 1), batch=3)")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_batch_384(knobs):
    """the resident kernels' 128-VGPR build; 384 workgroups of k_probe_record"""
    run_gpu(f"check_batch_384({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_closed_form_trapezoid(knobs):
    run_gpu(f"check_closed_pulse({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_closed_form_sampled_sine(knobs):
    run_gpu(f"check_closed_sine({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_sample_buffer_and_batch_independence(knobs):
    run_gpu(f"check_sample_buffer({knobs!r}, 'MI355X'); T.check_batch({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_window_rules(knobs):
    run_gpu(f"check_window_rules({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_adaptive_rejected_steps_record_nothing(knobs):
    run_gpu(f"check_adaptive_rejections({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_series_arm_at_tiny_steps(knobs):
    run_gpu(f"check_tiny_steps({knobs!r}, 'MI355X')")


@pytest.mark.parametrize("knobs", SCHEDULES[:2], ids=IDS[:2])
def test_compensated_sum_long_run(knobs):
    run_gpu(f"check_compensation({knobs!r}, 'MI355X')")


def test_refusals():
    run_gpu("check_refusals({'SPLIT': 0}, 'MI355X')")


def test_cpp_plug_in_api():
    """tests/cpp/fourier_rectifier.cpp against the product library: THD of the rectifier against the value the Python reference gives for
    the same run of the same library, within the propagated bound; the harmonics of pulse_src against the closed form"""
    from parity_common import make
    out = run_gpu("__name__; print('MI355X EXPECT %.17g %.17g' % T.cpp_expectations({'SPLIT': 0}, 'MI355X'))")
    thd, bound = next(line.split()[2:4] for line in out.splitlines() if line.startswith("MI355X EXPECT"))
    cpp = os.path.join(ROOT, "tests", "cpp")
    make("-C", cpp, "_build/fourier_rectifier")
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    r = subprocess.run([os.path.join(cpp, "_build", "fourier_rectifier"), thd, bound], capture_output=True, text=True, timeout=120)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, f"fourier_rectifier exited {r.returncode}: {r.stdout} {r.stderr}"
