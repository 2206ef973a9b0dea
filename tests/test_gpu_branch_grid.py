"""GPU (MI355X): the multifrontal LU on branch-heavy circuits.  The grids of tests/branch_grid_common.py -- half of the horizontal links
inductors, controlled sources, transformers and op-amp followers sprinkled over them: a third of the rows branch rows, an unsymmetric
pattern, a row matching that moves 70 % of the rows at DC -- through the DC solve (batches 1 and 5, every instance its own R and L), the
first transient step at two step sizes, four transient steps against the oracle with and without diodes, on the resident kernels and the
split schedule with and without captured graphs (W = 24) and on the lane-group / per-instance paths of the split schedule (W = 44), with
the static fronts skipped and not, and through the two solver seams.  Every instance solved is judged for (f) no silent error -- a status
of OK comes with a solution within tolerance -- and for being solved at all: these are systems plain LU solves to 1e-8 tolerance units.
tests/test_branch_grid_emu.py runs the same checks on the host emulation.

Every case is a child process of its own under a time limit; once a child has died of a signal or run out of time nothing more is started
on the GPU (the remaining cases fail without running)."""
import os
import subprocess
import sys

import pytest

import branch_grid_common as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = f"""
import os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import pe_load
import branch_grid_common as G
O = pe_load.load_oracle()
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
@pytest.mark.parametrize("knobs", G.SCHEDULES_24, ids=G.IDS_24)
@pytest.mark.parametrize("seed", G.SEEDS[24])
def test_dc_first_step_and_four_steps_24(seed, knobs):
    assert "BRANCH GRID OK" in run_gpu(f"G.check_all({knobs!r}, 24, {seed}, O, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", G.VARIANTS_44, ids=G.IDS_44)
@pytest.mark.parametrize("seed", G.SEEDS[44])
def test_dc_first_step_and_four_steps_44(seed, knobs):
    assert "BRANCH GRID OK" in run_gpu(f"G.check_all({knobs!r}, 44, {seed}, O, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", G.SEEDS[44])
def test_static_skip_is_bit_identical_44(seed):
    assert "BRANCH GRID OK" in run_gpu(f"G.check_static_skip(44, {seed}, O, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("W,seed", [(W, s) for W in G.SEEDS for s in G.SEEDS[W]])
def test_solver_seams(W, seed):
    assert "BRANCH GRID OK" in run_gpu(f"G.check_seams({W}, {seed}, 'MI355X')")


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.AC_GOLDENS)
def test_ac_stamps_through_the_complex_seam(name):
    assert "BRANCH GRID OK" in run_gpu(f"G.check_ac_stamps({name!r}, O, 'MI355X')")
