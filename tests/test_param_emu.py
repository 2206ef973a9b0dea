"""CPU: the checks of tests/test_gpu_param.py on the host emulation of the kernels (tests/emu), each in a child process with PE_HIP_LIB set.
Which instance's parameters reach a stamp, what pe_hip_update_param writes and what it invalidates, how a sweep slices its tables per
device and the column counts of the tables are host logic and index data: the emulation walks the same tables.  Here alone: the
deliberately wrong references of case 1 (they must fail for every kind), the two emulated devices of the shard case, and the pin of
ffi.NCOL to the library's column counts."""
import os
import subprocess
import sys

import pytest

from parity_common import ROOT, make

SCHEDULES = ['{"SPLIT": 0}', '{"SPLIT": 1, "GRAPH": 0}', '{"SPLIT": 1, "GRAPH": 1}']      # device_eval_common.SCHEDULES
IDS = ["resident", "split", "split_graph"]
ANALYSES = ["tr", "ac", "ac_sweep", "noise", "sens", "net", "pz", "dc_sweep", "dc_sweep_parallel"]      # param_common.STALE_ANALYSES


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
import param_common as P
{body}
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=600, env=dict(os.environ, **(env or {})))


def test_lists_match_the_shared_module():
    import param_common as P
    assert [eval(s) for s in SCHEDULES] == P.SCHEDULES and ANALYSES == list(P.STALE_ANALYSES)


def test_tables_cover_every_kind_and_column_and_the_reference_converges(oracle_mod):
    """all_overrides asserts the distinct values, check_coverage every (kind, column) of ffi.NCOL; the spreads' condition: the float64
    oracle converges from x = 0 at the operating point for all five instances"""
    import param_common as P
    for B in (3, 5):
        deck, ov, _ = P.case(B)
        assert set(ov) == set(P.F.NCOL)
    P.check_reference_converges(oracle_mod, 5)


def test_short_table_is_refused():
    import param_common as P
    P.check_short_table_refused()


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_load_time_tables_match_each_instances_own_deck(emu_lib, knobs):
    run_emu(emu_lib, f"P.check_load_bitwise({knobs}, {knobs!r})")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_load_time_tables_against_references_and_wrong_references_fail(emu_lib, knobs):
    run_emu(emu_lib, f"P.check_load_references({knobs}, {knobs!r}, wrong=True)")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_load_time_tables_ac_side(emu_lib, knobs):
    run_emu(emu_lib, f"P.check_ac({knobs}, {knobs!r})")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_update_param_equals_a_fresh_load(emu_lib, knobs):
    run_emu(emu_lib, f"P.check_update_equals_load({knobs}, {knobs!r})")


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_update_param_changes_one_device_of_one_instance(emu_lib, knobs):
    run_emu(emu_lib, f"P.check_update_locality({knobs}, {knobs!r})")


@pytest.mark.parametrize("analysis", ANALYSES)
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_nothing_stale_after_update_param(emu_lib, knobs, analysis):
    run_emu(emu_lib, f"P.check_nothing_stale({knobs}, {analysis!r}, {knobs!r})")


def test_nothing_stale_after_update_param_on_the_lane_group_mesh(emu_lib):
    run_emu(emu_lib, "P.check_nothing_stale_mesh()")


def test_shards_read_their_instances_tables(emu_lib):
    run_emu(emu_lib, "P.check_shards()", {"PE_EMU_DEVICES": "2"})


def test_column_counts_match_the_library(emu_lib):
    run_emu(emu_lib, "P.check_column_counts(True)", {"PE_EMU_DEVICES": "2"})
