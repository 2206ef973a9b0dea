"""CPU: the oracle (oracle/pe_oracle.py) against golden vectors captured from the REAL reference
(scripts/make_golden.py -> oracle/_ref/ref_driver) and against the known answers of the reference's own tests."""
import math

import numpy as np
import pytest

from parity_common import golden, golden_complex

FAST = ["rc_step", "rl_step", "rlc_series_vl", "rlc_series_vl_trop", "divider_dc", "diode_op", "pn_tt_tr", "ladder_c1", "bridge_c2",
        "mesh32_lin", "mesh32_nl", "mesh32_lin_seed3", "mesh32_nl_seed7"]
# the remaining linear stampers (goldens from the reference's own model tests + transient variants)
STAMPERS = ["vccs_dc", "vcvs_gain", "cccs_dc", "ccvs_dc", "op_amp_follower", "transformer_ratio", "generator_dc", "switch_open_dc",
            "switch_closed_dc", "switch_open_ropen1e6_dc", "generators_tr", "generators_trop", "iac_rc_tr", "iac_rc_dc", "iac_rc_trop",
            "coupled_l_k0_tr", "coupled_l_k09_tr", "coupled_l_k09_trop", "coupled_l_dc", "controlled_mix_tr",
            "nmos_cutoff_dc", "nmos_sat_dc", "nmos_triode_op", "cmos_inverter_tr", "bjt_amp_tr", "center_tap_ratio", "relay_ramp_tr"]


def run_oracle(orc, meta, deck):
    o = orc.Oracle(deck, g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
    if meta["analysis"] in ("DC", "OP"):
        o.analyze_dc(meta["analysis"])
        return o, np.array([o.x])
    out = o.analyze_tr(meta["dt"], meta["steps"], set(meta["snap_steps"]), trop=meta["analysis"] == "TROP")
    return o, np.array([out[s] for s in meta["snap_steps"] if s in out])


@pytest.mark.parametrize("name", FAST + STAMPERS)
def test_oracle_matches_reference_golden(oracle_mod, name):
    meta, gx, deck = golden(name)
    o, xs = run_oracle(oracle_mod, meta, deck)
    assert len(xs) == len(gx)
    # fp64, same algorithm family (SuperLU vs Eigen's SuperLU port): 1e-9 abs + 1e-9 rel
    assert np.all(np.abs(xs - gx) <= 1e-9 + 1e-9 * np.abs(gx))
    assert o.newton_iters == meta["newton_iters"]


@pytest.mark.parametrize("name", ["bjt_npn_ce_dc_fail", "bjt_pnp_ce_op_fail", "bjt_amp_trop_fail"])
def test_oracle_unlimited_exponential_fails_like_reference(oracle_mod, name):
    """The reference's BJT has a plain exp without junction limiting (BJT_NPN.h:128): a cold-start operating point
    overflows and Newton gives up after 64 iterations.  Same behaviour required, not a 'better' answer."""
    meta, gx, deck = golden(name)
    assert meta["fail_step"] == 0 and meta["newton_iters"] == [-2]
    o = oracle_mod.Oracle(deck, g_min=meta["gmin"])
    with np.errstate(all="ignore"):
        if meta["analysis"] == "TROP":
            o.analyze_tr(meta["dt"], meta["steps"], set(), trop=True)
            assert o.fail_step == 0
        else:
            assert not o.analyze_dc(meta["analysis"])
    assert o.newton_iters[0] < 0


AC_CASES = ["ac_rc_lowpass", "ac_rlc_diode_acop", "ac_linear_mix", "ac_nmos_amp", "ac_controlled_rest_acop", "ac_transistors_acop", "ac_transistors_hf_acop"]


@pytest.mark.parametrize("name", AC_CASES)
def test_oracle_ac_matches_reference_golden(oracle_mod, name):
    """Small-signal AC: complex phasors of every node voltage / branch current per frequency point."""
    meta, gx, deck = golden(name)
    o = oracle_mod.Oracle(deck, g_min=meta["gmin"])
    xs = o.analyze_ac(meta["omegas"], acop=meta["analysis"] == "ACOP")
    g = golden_complex(meta, gx)
    assert xs is not None and len(xs) == len(g)
    for x, gg in zip(xs, g):
        assert np.all(np.abs(x - gg) <= 1e-9 + 1e-7 * np.abs(gg))


def test_known_answer_ac_lowpass(oracle_mod, pe):
    """test/0012.ac/ac_omega.cpp: |v_out| in (0.6, 0.8) at omega = 1 / (R C) -- exactly 1 / sqrt(2)."""
    o = oracle_mod.Oracle(pe.deck.ac_rc_lowpass())
    x = o.analyze_ac([1000.0])[0]
    assert abs(abs(x[1]) - 1.0 / math.sqrt(2.0)) < 1e-12


def test_oracle_mesh100_first_steps(oracle_mod):
    meta, gx, deck = golden("mesh100_nl")
    o = oracle_mod.Oracle(deck)
    out = o.analyze_tr(meta["dt"], 10, {1, 10})
    for k, s in enumerate((1, 10)):
        assert np.all(np.abs(out[s] - gx[k]) <= 1e-9 + 1e-9 * np.abs(gx[k]))
    assert o.newton_iters == meta["newton_iters"][:10]


def test_bridge_gmin0_fails_like_reference(oracle_mod):
    """With g_min = 0 the bridge goes singular when all four diodes are off: the reference fails at
    step 80; the exact step is implementation-defined (near-singular pivot), so accept a small window."""
    meta, gx, deck = golden("bridge_gmin0_fail")
    o = oracle_mod.Oracle(deck, g_min=0.0)
    out = o.analyze_tr(meta["dt"], meta["steps"], {50})
    assert np.all(np.abs(out[50] - gx[0]) <= 1e-9 + 1e-9 * np.abs(gx[0]))
    assert meta["fail_step"] == 80 and 76 <= o.fail_step <= 82


# ---- known answers held by the reference's own tests -------------------------------------------------------
def test_known_answer_rc_step(oracle_mod, pe):
    """test/0005.models/rc_step_tr.cpp:59-61: |v - (1 - e^-1)| <= 5e-3 after 100 trapezoidal steps."""
    o = oracle_mod.Oracle(pe.deck.rc_step())
    o.analyze_tr(1e-8, 100)
    assert abs(o.x[1] - (1.0 - math.exp(-1.0))) <= 5e-3


def test_known_answer_divider(oracle_mod, pe):
    """test/0004.solver/dc.cpp: 3 V / (10 + 20) ohm -> node voltages 2 V, 3 V, source current 0.1 A."""
    o = oracle_mod.Oracle(pe.deck.divider_dc())
    assert o.analyze_dc("DC")
    assert np.allclose(o.x, [2.0, 3.0, -0.1], atol=1e-12)


def test_known_answer_diode_op(oracle_mod, pe):
    """test/0011.nonlinear/op_pn_junction.cpp:27-30: Newton converges with 0.5 V < Vd < 0.9 V."""
    o = oracle_mod.Oracle(pe.deck.diode_op())
    assert o.analyze_dc("OP")
    assert 0.5 < o.x[1] < 0.9


def test_known_answer_trapezoid_closed_form(oracle_mod, pe):
    """test/0008.numerical_methods/compare_trapezoidal_vs_backward_euler.cpp:35-66: RC (1k, 1uF, 5 V), dt 1e-4:
    v[n+1] = ((1 - a) v[n] + 2 a Vs) / (1 + a), a = dt / (2 R C), from the second step on (the engine's first
    step starts from zero companion history, capacitor.h:124)."""
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VDC", (1, 0), 5.0)
    d.add("R", (1, 2), 1000.0)
    d.add("C", (2, 0), 1e-6)
    o = oracle_mod.Oracle(d)
    snaps = o.analyze_tr(1e-4, 100, set(range(1, 101)))
    a = 1e-4 / (2.0 * 1000.0 * 1e-6)
    for n in range(2, 100):
        v, vn = snaps[n][1], snaps[n + 1][1]
        assert abs(vn - ((1 - a) * v + 2 * a * 5.0) / (1 + a)) < 1e-12


def test_known_answer_pn_tt(oracle_mod):
    """test/0004.solver/pn_junction_tt_tr.cpp:54-58: the diffusion-cap companion changes the source current by > 1e-4 A."""
    meta, gx, deck = golden("pn_tt_tr")
    o1 = oracle_mod.Oracle(deck)
    o1.analyze_tr(1e-8, 2)
    d0 = type(deck).loads(deck.dumps())
    k, n, p = d0.devices[2]
    d0.devices[2] = (k, n, p[:9] + (0.0,))
    o0 = oracle_mod.Oracle(d0)
    o0.analyze_tr(1e-8, 2)
    assert abs(o1.x[3]) > abs(o0.x[3]) + 1e-4
