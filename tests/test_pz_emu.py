"""Pole-zero analysis (pe_hip_analyze_pz / pe_hip_get_pz* / pe_hip_eig_hessenberg, include/pe_hip.h) on the CPU: the engine's host logic and
the team- and wave-generic kernel text (pe_pz.hpp) through the host emulation library (tests/emu: test infrastructure), one child process
per case.  Truth (mpmath at 50 digits over the unchanged CPU oracle's stamps), the bound per value and the cases themselves:
tests/pz_common.py.  Every parity case asserts one factorisation and at least as many kept-factor solves as Arnoldi steps."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
CPP = os.path.join(ROOT, "tests", "cpp")
SCRIPTS = os.path.join(ROOT, "scripts")


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
import pz_common as P
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-3000:])
    return r.stdout


@pytest.mark.parametrize("split", [0, 1])
def test_known_answers(emu, split):
    """R C low pass (one pole, complete after one step), series R L C (two real poles; a complex pair in the order of the rule), an R C lead
    network (one closed-form zero, a voltage excitation through the source's branch row)"""
    run(emu, "P.known_answers(pe, O, {'SPLIT': %d})\n" % split)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", ["ac_linear_mix", "ac_rlc_diode", "ac_nmos_amp", "ac_controlled_rest", "ac_transistors"])
def test_parity_of_poles(emu, name, split):
    """complete, as many poles as the reference has finite ones, each within its bound; one factorisation"""
    run(emu, "P.parity(pe, O, %r, {'SPLIT': %d})\n" % (name, split))


def test_instances_finish_at_different_steps(emu):
    """batch 3 of ac_linear_mix, one instance a pole short: parked first, and bit for bit what it is alone at batch 1"""
    run(emu, "P.different_steps(pe, O)\n")


def test_mesh6_poles_zeros_and_gain(emu):
    """rc_mesh(6, 6, 1, True) at batch 3, 64 steps: complete with 36 poles; zeros of (1, -1) -> (30, 17); H(s0) against the network analysis"""
    run(emu, "P.mesh6(pe, O)\n")


def test_mesh16_nearest_poles_in_order(emu):
    """rc_mesh(16, 16, 1, True) at omega0 = 1e8, 32 and 64 steps: not complete, the leading converged run is the fixture's nearest poles"""
    run(emu, "P.mesh16(pe, O)\n")


def test_determinism(emu):
    run(emu, "P.determinism(pe, O)\n")


def test_eig_hessenberg_alone(emu):
    """the Ritz kernel on caller-supplied matrices against mpmath: m = 1 .. 64, deflated, Jordan, repeated, scaled rows, NaN"""
    run(emu, "P.eig_cases(pe)\n")


def test_refusals_and_statuses(emu):
    run(emu, "P.refusals_and_statuses(pe, O)\n")


def test_plugin_api_under_host_emulation(emu):
    """tests/cpp/pz_rlc.cpp: circult::analyze_pz of the plug-in API on the series R L C against the closed form"""
    make("-C", CPP, "_build_emu/pz_rlc")
    out = subprocess.run([os.path.join(CPP, "_build_emu", "pz_rlc")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"pz_rlc exited {out.returncode}: {out.stdout} {out.stderr}"


def test_kernel_text_under_sanitizers(tmp_path):
    """scripts/pz_kernel_host.cpp: the text of pe_pz.hpp as a stand-alone host program, every buffer at exactly the engine's size, built
    with -fsanitize=address,undefined: no report, exit 0"""
    exe = str(tmp_path / "pz_kernel_host")
    src = os.path.join(SCRIPTS, "pz_kernel_host.cpp")
    inc = ["-I" + os.path.join(ROOT, "tests", "emu", "hip_shim"), "-I" + os.path.join(ROOT, "phy-engine_amd", "csrc")]
    b = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *inc, "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, (out.stdout[-2000:], out.stderr[-4000:])
