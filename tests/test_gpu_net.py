"""GPU (MI355X): multi-port network analysis (pe_hip_analyze_net / pe_hip_get_net* / pe_hip_convert_net, include/pe_hip.h) -- one
factorisation per pass and kept-factor solves for the further ports, columns by k_net_gather, Y and S by k_net_convert (one wavefront per
matrix) -- against the CPU oracle and mpmath.  The cases, the reference and the derived tolerances are those of the emulation test:
tests/net_common.py.  Knob SPLIT at 0 and 1, NET_POINTS at 1, 4 and automatic."""
import os
import subprocess

import pytest

import net_common as N
from parity_common import ROOT, make, pe

pytestmark = pytest.mark.gpu

CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("points", [1, 4, None])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", N.PARITY)
def test_parity(oracle_mod, name, split, points):
    """Z, Y and S against the oracle within the propagated tolerance; n_factorisations == n_passes: a build that factors per port fails"""
    N.parity(pe, oracle_mod, name, {"SPLIT": split, "NET_POINTS": points})


@pytest.mark.parametrize("split", [0, 1])
def test_known_answers(oracle_mod, split):
    N.known_answers(pe, oracle_mod, {"SPLIT": split})


@pytest.mark.parametrize("split", [0, 1])
def test_properties(oracle_mod, split):
    N.properties(pe, oracle_mod, {"SPLIT": split})


def test_conversion_at_its_edges():
    """k_net_convert against mpmath at 50 digits: tail and full workgroups, forced row exchanges, singular and NaN matrices"""
    N.conversion_edges(pe)


def test_refusals_state_and_failures(oracle_mod):
    N.refusals_state_failures(pe, oracle_mod)


def test_calls_of_different_shapes_on_one_engine(oracle_mod):
    """result planes of equal size, status arrays of different size: 8 ports x 1 point, then 1 port x 64 points on the same engine"""
    N.shapes_on_one_engine(pe, oracle_mod)


def test_plugin_api():
    """tests/cpp/net_twoport.cpp: circult::analyze_net on an R - C low pass against the closed form"""
    make("-C", CPP, "_build/net_twoport")
    out = subprocess.run([os.path.join(CPP, "_build", "net_twoport")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"net_twoport exited {out.returncode}: {out.stdout} {out.stderr}"
