"""GPU (MI355X): the Newton iterations after the first of a solve point skip the static fronts of the lane-group kernel --
k_m2_factor_quads on the program without them, their roots' update matrices in persistent arena slots, their forward-substituted pivots put
back by the stamp.  Nothing may change but the time: every run is compared bit for bit with STATIC_SKIP = 0 on the 56 x 56 diode mesh (the
smallest on the split schedule with the lane-group kernel), batch 5 = a full quad + a quad with three invalid lanes.
tests/test_static_skip_emu.py runs the same checks on the host emulation."""
import os
import subprocess
import sys

import pytest

import static_skip_common as S
from parity_common import ROOT

pytestmark = pytest.mark.gpu


def test_bit_identity():
    S.check_bit_identity()


def test_bit_identity_many_children():
    S.check_bit_identity(S.KNOBS_MANY_CHILDREN, "many children")


def test_bit_identity_captured_sequences():
    S.check_bit_identity({"GRAPH": 1}, "captured sequences")


def test_classification_reaches_every_case():
    S.check_classification()


def test_instances_leaving_mid_point():
    S.check_leaving()


def test_refinement_ends_the_skip():
    S.check_refinement()


def test_fallback_linear_deck():
    S.check_linear()


def test_fallback_host_stamp_overlay():
    S.check_overlay()


def test_fallback_full_stamp():
    """(PHY_ENGINE_HIP_FULL_STAMP is read once per process: a child process, which is what this test is about)"""
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import static_skip_common as S; S.check_full_stamp()"
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120, env=dict(os.environ, PHY_ENGINE_HIP_FULL_STAMP="1"))
