"""GPU (MI355X): instance b of a batch reads its own parameters for every device of every kind on every path, and pe_hip_update_param
changes exactly one (device, column, instance) and leaves nothing stale (tests/param_common.py).  Every comparison is for bit
identity between two routes to the same numbers, or goes through the references and bounds of device_eval_common / ac_stamp_common.
tests/test_param_emu.py runs the same checks on the host emulation, and there the deliberately wrong references."""
import pytest

import param_common as P

pytestmark = pytest.mark.gpu
IDS = ["resident", "split", "split_graph"]


@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_load_time_tables_match_each_instances_own_deck(knobs):
    P.check_load_bitwise(knobs, str(knobs))


@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_load_time_tables_against_references(knobs):
    P.check_load_references(knobs, str(knobs))


@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_load_time_tables_ac_side(knobs):
    P.check_ac(knobs, str(knobs))


@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_update_param_equals_a_fresh_load(knobs):
    P.check_update_equals_load(knobs, str(knobs))


@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_update_param_changes_one_device_of_one_instance(knobs):
    P.check_update_locality(knobs, str(knobs))


@pytest.mark.parametrize("analysis", list(P.STALE_ANALYSES))
@pytest.mark.parametrize("knobs", P.SCHEDULES, ids=IDS)
def test_nothing_stale_after_update_param(knobs, analysis):
    P.check_nothing_stale(knobs, analysis, str(knobs))


def test_nothing_stale_after_update_param_on_the_lane_group_mesh():
    P.check_nothing_stale_mesh()


def test_shards_read_their_instances_tables():
    if P.F.lib().pe_hip_device_count() < 2:
        pytest.skip("one device visible: the sharded sweep needs two")
    P.check_shards()


def test_column_counts_on_one_device():
    P.check_column_counts(False)
