"""Multi-port network analysis (pe_hip_analyze_net / pe_hip_get_net* / pe_hip_convert_net, include/pe_hip.h) on the CPU: the engine's host
logic and the team-generic kernel text (pe_net.hpp) through the host emulation library (tests/emu: test infrastructure), one child process
per case.  Reference, tolerances and the cases themselves: tests/net_common.py (the unchanged CPU oracle; the project's AC tolerance
propagated to Z, Y and S; mpmath for the conversion alone).  Every parity case asserts n_retried_points == 0 and one factorisation per
pass."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


PRE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import pe_load
pe = pe_load.load()
O = pe_load.load_oracle()
import net_common as N
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    e.pop("PHY_ENGINE_HIP_NET_POINTS", None)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-3000:])
    return r.stdout


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", ["ac_linear_mix", "ac_nmos_amp", "mesh6_batch3", "mesh16_ports8"])
def test_parity(emu, name, split):
    """Z, Y and S against the oracle within the propagated tolerance, on both schedules; one factorisation per pass"""
    run(emu, "for P in (1, 4, None):\n    N.parity(pe, O, %r, {'SPLIT': %d, 'NET_POINTS': P})\n" % (name, split))


@pytest.mark.parametrize("split", [0, 1])
def test_known_answers(emu, split):
    """R - C low pass as a one-port (closed form), with a port on the node the source holds (Y singular, S fine), a matched resistor"""
    run(emu, "N.known_answers(pe, O, {'SPLIT': %d})\n" % split)


def test_properties(emu):
    """reciprocity and passivity within the propagated bound; bit-identical across the pass size, batch positions and a port permutation"""
    run(emu, "N.properties(pe, O)\n")


def test_conversion_at_its_edges(emu):
    """pe_hip_convert_net against mpmath at 50 digits: n = 1, 2, 3, 8, row scaling, forced row exchanges, singular and NaN matrices"""
    run(emu, "N.conversion_edges(pe)\n")


def test_refusals_state_and_failures(emu):
    run(emu, "N.refusals_state_failures(pe, O)\n")


def test_calls_of_different_shapes_on_one_engine(emu):
    """result planes of equal size, status arrays of different size: 8 ports x 1 point, then 1 port x 64 points on the same engine"""
    run(emu, "N.shapes_on_one_engine(pe, O)\n")


def test_touchstone_round_trip(tmp_path):
    """ffi.write_touchstone: a file parsed back reads the arrays exactly; unequal reference resistances raise ValueError"""
    from parity_common import pe
    import net_common as N
    N.touchstone_round_trip(pe, str(tmp_path))


def test_plugin_api_under_host_emulation(emu):
    """tests/cpp/net_twoport.cpp: circult::analyze_net of the plug-in API on an R - C low pass against the closed form"""
    make("-C", CPP, "_build_emu/net_twoport")
    out = subprocess.run([os.path.join(CPP, "_build_emu", "net_twoport")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"net_twoport exited {out.returncode}: {out.stdout} {out.stderr}"
