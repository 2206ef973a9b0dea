"""GPU (MI355X): the multifrontal LU at the edges of every front class.  The circuits of tests/front_shapes_common.py put fronts ON the
integer limits the symbolic analysis sorts them by -- lane-group kernel: order 16 / 17 / 32 / 33, 16 pivots, 255 / 256 own entries, 16 / 17
children, partial quads; per-instance wave fronts: whole in the slot / panel layout; cooperative fronts: whole, panels + pull, chain links;
the resident kernel's limits through the solver seams -- and every test asserts through Engine.front_table() that it reached the classes
it exists for.  A linear DC solve is one stamp, one factorisation and one forward / backward pass: what is compared with the
high-precision reference is the LU kernels.  tests/test_front_shapes_emu.py runs the same checks on the host emulation."""
import pytest

import front_shapes_common as F

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    e = F.new_engine()
    yield e
    e.close()


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 7])
def test_parity_per_instance(eng, batch):
    """partial quads (1, 2, 3 live slots), a full quad + 1, a full quad + 3: every instance its own matrix"""
    F.check_parity(eng, batch)


def test_many_children():
    e = F.new_engine(F.KNOBS_MANY_CHILDREN)
    try:
        F.check_parity(e, 3, F.DEFAULT_CLASSES + F.KNOB_CLASSES, "many children")
    finally:
        e.close()


def test_slot_independence(eng):
    F.check_slot_independence(eng)


def test_launch_variants_are_bit_identical():
    F.check_launch_variants()


def test_one_bad_instance_in_a_quad(eng):
    F.check_one_bad_instance(eng)


def test_transient_step_after_dc(eng, oracle_mod):
    F.check_transient_step(eng, oracle_mod)


@pytest.fixture
def seam_eng():
    e = F.pe.ffi.Engine(device=0)
    yield e
    e.close()


@pytest.mark.parametrize("name", ["chain200", "chain100"])
def test_real_seam_patterns(seam_eng, name):
    F.check_real_seam(seam_eng, name)


def test_complex_seam_pattern(seam_eng):
    F.check_complex_seam(seam_eng, "chain100")
