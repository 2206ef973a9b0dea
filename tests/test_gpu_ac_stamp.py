"""The small-signal systems on the MI355X against the mpmath restatement of tests/ac_stamp_common.py: the checks of
tests/test_ac_stamp_emu.py on the real library, where k_ac_sweep_fill runs its grid-strided loops over more value slots than a workgroup has
threads, k_ac_residual / k_ac_residual_each reduce the backward error across waves, and the solves are the device's.  Every case is a child
process of its own under a time limit; once a child has died of a signal or run out of time nothing more is started on the GPU (the
remaining cases fail without running)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import ac_stamp_common as A
"""

_gpu_lost = []


def run_gpu(body, timeout=120):
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    try:
        r = subprocess.run([sys.executable, "-c", PRE + body], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _gpu_lost.append("time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    print(r.stdout)
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("g_min", [0.0, 2.0 ** -40], ids=["gmin0", "gmin"])
def test_one_device_per_deck(g_min):
    assert "RATIOS" in run_gpu(f"A.check_single({{}}, 'MI355X', {g_min!r})")


@pytest.mark.gpu
def test_infinite_inductor_at_omega_zero():
    assert "RATIOS" in run_gpu("A.check_inf_inductor({}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True], ids=["one_block", "five_blocks"])
@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}], ids=["resident", "split"])
def test_mixed_deck(knobs, big):
    assert "RATIOS" in run_gpu(f"A.check_mixed({knobs!r}, 'MI355X', big={big!r})")


@pytest.mark.gpu
def test_adjoint_system():
    assert "RATIOS" in run_gpu("A.check_adjoint({}, 'MI355X')")


@pytest.mark.gpu
def test_nan_instance():
    assert "RATIOS" in run_gpu("A.check_nan_instance({}, 'MI355X')")


@pytest.mark.gpu
def test_band_edge():
    assert "RATIOS" in run_gpu("A.check_band_edge({}, 'MI355X')")
