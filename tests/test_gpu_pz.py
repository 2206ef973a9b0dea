"""GPU (MI355X): pole-zero analysis (pe_hip_analyze_pz / pe_hip_get_pz* / pe_hip_eig_hessenberg, include/pe_hip.h) -- one factorisation,
every Arnoldi step a kept-factor solve between k_pz_bmul and k_pz_orth (one workgroup per instance), Ritz values by k_pz_ritz (one wavefront
per matrix, the matrix in LDS) -- against mpmath at 50 digits.  The cases, the truth and the bound per value are those of the emulation
test: tests/pz_common.py.  Knob SPLIT at 0 and 1."""
import os
import subprocess

import pytest

import pz_common as P
from parity_common import ROOT, make, pe

pytestmark = pytest.mark.gpu

CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("split", [0, 1])
def test_known_answers(oracle_mod, split):
    P.known_answers(pe, oracle_mod, {"SPLIT": split})


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", list(P.PARITY))
def test_parity_of_poles(oracle_mod, name, split):
    """complete, as many poles as the reference has finite ones, each within its bound; n_factorisations == 1: a build that factors per step fails"""
    P.parity(pe, oracle_mod, name, {"SPLIT": split})


def test_instances_finish_at_different_steps(oracle_mod):
    P.different_steps(pe, oracle_mod)


def test_mesh6_poles_zeros_and_gain(oracle_mod):
    """76 real rows: less than one stride of k_pz_orth's workgroup; Hessenberg matrices of order 36 and 37"""
    P.mesh6(pe, oracle_mod)


def test_mesh16_nearest_poles_in_order(oracle_mod):
    """516 real rows: the sums of k_pz_orth cross their stride; k_pz_ritz at m = 32 and at m = 64 (the whole LDS allotment)"""
    P.mesh16(pe, oracle_mod)


def test_determinism(oracle_mod):
    P.determinism(pe, oracle_mod)


def test_eig_hessenberg_alone():
    """k_pz_ritz against mpmath: m = 1, 2, 3, 31, 32, 33, 64; 1, 5 and 65 matrices per launch; deflated, Jordan, repeated, scaled rows, NaN"""
    P.eig_cases(pe)


def test_refusals_and_statuses(oracle_mod):
    P.refusals_and_statuses(pe, oracle_mod)


def test_plugin_api():
    """tests/cpp/pz_rlc.cpp: circult::analyze_pz on the series R L C against the closed form"""
    make("-C", CPP, "_build/pz_rlc")
    out = subprocess.run([os.path.join(CPP, "_build", "pz_rlc")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"pz_rlc exited {out.returncode}: {out.stdout} {out.stderr}"
