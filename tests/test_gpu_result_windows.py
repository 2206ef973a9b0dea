"""GPU (MI355X): the window check of the stored-result getters at its edges, and what makes a stored result unreadable.  The cases are
those of the emulation test: tests/result_windows_common.py."""
import pytest

import result_windows_common as RW
from parity_common import pe

pytestmark = pytest.mark.gpu


def test_windows():
    """every getter, every combination of the nine (first, n) and the nine (first_instance, count) pairs, sentinel-filled buffers"""
    RW.check_windows(pe)


def test_validity():
    """pe_hip_update_param and pe_hip_set_dc_sweep_rows: every getter answers with its own "no ... yet" """
    RW.check_validity(pe)
