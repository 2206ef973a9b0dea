"""Shared bodies of the tests of the Fourier analysis of transient probes (pe_hip_set_fourier / pe_hip_get_fourier, include/pe_hip.h):
tests/test_fourier_emu.py runs them on the host emulation, one child process per case, tests/test_gpu_fourier.py on the device -- there
the 64-lane workgroup of k_probe_record, the 512-thread workgroup of the resident kernel, the device's libm and k_fourier_finish are
what is added.

The reference is never the engine under test.  reference() integrates, in mpmath at 256 bits, the piecewise-linear interpolant through
THE ENGINE'S OWN ACCEPTED POINTS (read back with stride 1 and capacity >= steps + 1) over the clipped window, with the antiderivative
of (alpha + beta tau) e^{-j w tau} taken at the segment's two ends -- not the midpoint form of pe_fourier.hpp.  The closed forms of
check 2 do not use the step sequence at all.

The tolerance is a running first-order rounding bound, accumulated segment by segment beside the reference (u = 2^-53 per rounded
operation, terms of order u^2 dropped except where named).  With ~ marking the computed value, per accepted step and harmonic k:
  tau_a, tau_b   one subtraction each                         d_tau  <= u |tau|   (0 where t_start == 0: the subtraction is exact)
  h              tau_b - tau_a                                d_h    <= d_tau_a + d_tau_b + u h
  tau_m          fma(0.5, h, tau_a)                           d_taum <= d_tau_a + d_h / 2 + u |tau_m|
  w              k * (2 pi * f0): constant, 2 products        3 u relative
  arg            w * tau_m                                    d_arg  <= w d_taum + 4 u |w tau_m|      (the sincos argument: amplified by |k w0 tau|)
  cos, sin       libm within 1 ulp: 2 u per call              d_cs   <= d_arg + 2 u
  phi            0.5 * w * h                                  d_phi  <= w d_h / 2 + 4 u phi
  A = sin phi / phi        dA/dphi = -2 B                     d_A    <= 4 u |A| + 2 |B| d_phi         (either arm: 2 u libm + division / 7 fma)
  B = (sin phi - phi cos phi) / (2 phi^2)   dB/dphi = A / 2 - 2 B / phi
                                                              d_B    <= 4 u |B| + |A / 2 - 2 B / phi| d_phi
                                                                        + [closed arm] 2 u (|phi cos phi| + |sin phi|) / (2 phi^2)
  va, vb         exact unless clipped; clipped: fma(v1 - v0, r, v0), r a quotient of differences
                                                              d_v    <= 4 u |v1 - v0| + u |v|
  vm, d          (va + vb) / 2, vb - va                       d_vm   <= (d_va + d_vb) / 2 + u |vm|;  d_d <= d_va + d_vb + u |d|
  pa = vm A, pb = d B                                         d_pa   <= |A| d_vm + |vm| d_A + u |pa|;  d_pb likewise
  c = h fma(pa, cos, -(pb sin))                               d_c    <= |inner| d_h + h (|cos| d_pa + |sin| d_pb + (|pa| + |pb|) d_cs
                                                                        + u |pb sin| + u |inner|) + u |c|            (s likewise)
  k = 0: A = 1, B = 0, cos = 1, sin = 0 exactly: only the v, h and product terms remain.
The compensated sum (TwoSum cascade, Ogita / Rump / Oishi Sum2) adds u |C| for the final sum + compensation and (n u)^2 sum |c_i|:
to first order a term independent of the number of steps n.  a_k = (2 C) / Tw adds 2 u |a_k| (Tw is one subtraction of the two
doubles the host passes; the reference takes those doubles as exact).  Propagated: amp = sqrt(fma(a, a, b b)): (|a| d_a + |b| d_b) / amp +
2 u amp; phase = atan2: (|a| d_b + |b| d_a) / amp^2 + 2 u |phase|; thd: the sum of squares gathers 2 amp d_amp + (H - 1) u sum, then
sqrt and the division: d_sum / (2 sqrt(sum) amp_1) + thd d_amp_1 / amp_1 + 2 u thd.

Every case asserts that the fundamental and at least one harmonic k >= 2 exceed 1000 x their bound: the bound cannot swallow a wrong
coefficient.  Worst |error| / bound per deck is printed ("FOURIER <where> worst ...") and recorded in DESIGN.md."""
import math

import mpmath as mp
import numpy as np

from parity_common import pe

F, D = pe.ffi, pe.deck
mp.mp.prec = 256
U = 2.0 ** -53
F0 = 1e3
T0 = 1.0 / F0
SERIES_BELOW = 0.25  # pe::FOURIER_SERIES_BELOW


# ---------------------------------------------------------------------------------------------------------------- decks
def pulse_src():
    d = D.Deck()
    n = d.new_node()
    d.add("PULSE", (n, 0), 1.0, 0.0, F0, 0.5, 0.0, T0 / 8, T0 / 8)
    d.add("R", (n, 0), 1e3)
    return d


def vac_r():
    d = D.Deck()
    n = d.new_node()
    d.add("VAC", (n, 0), 1.0, 2.0 * math.pi * F0, 0.0)
    d.add("R", (n, 0), 1e3)
    return d


def rectifier():
    d = D.Deck()
    a, k = d.new_node(), d.new_node()
    d.add("VAC", (a, 0), 2.0, 2.0 * math.pi * F0, 0.0)
    d.add("D", (a, k))
    d.add("R", (k, 0), 1e3)
    d.add("C", (k, 0), 1e-6)
    return d


# name -> (deck, g_min, probe rows, the amplitude as pe_hip_update_param names it, its load-time value)
DECKS = {
    "pulse_src": (pulse_src, 0.0, [0, 1], (F.VGEN, 0, 1), 1.0),
    "vac_r": (vac_r, 0.0, [0, 1], (F.VAC, 0, 0), 1.0),
    "rectifier": (rectifier, 1e-12, [1, 0, 2], (F.VAC, 0, 0), 2.0),
    "pulse_rc": (D.pulse_rc, 0.0, [1, 0], (F.VGEN, 0, 1), 5.0),
}
AMPS3 = [1.0, 0.5, 1.5]  # batch 3: factors on the load-time amplitude


def engine(name, knobs=None, batch=1, amps=None, **opt):
    deck, gmin, rows, par, a0 = DECKS[name]
    e = F.Engine()
    e.set_options(g_min=gmin, **opt)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck(), batch, None)
    e.reset()
    if amps is not None:
        e.update_param(par[0], par[1], par[2], [a0 * f for f in amps] if batch > 1 else [a0 * amps[0]])
    return e


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- reference and bound
def weights(phi):
    """A, B of pe_fourier.hpp in double (for the bound's magnitudes only), vector over k"""
    phi = np.asarray(phi, dtype=float)
    q = phi * phi
    with np.errstate(all="ignore"):
        a_c = np.where(phi != 0, np.sin(phi) / np.where(phi != 0, phi, 1.0), 1.0)
        b_c = np.where(phi != 0, (np.sin(phi) - phi * np.cos(phi)) / np.where(phi != 0, 2.0 * q, 1.0), 0.0)
    b_s = phi * (1.0 / 6 - q / 60 + q * q / 1680)
    return a_c, np.where(np.abs(phi) < SERIES_BELOW, b_s, b_c)


class Ref:
    pass


def reference(t, v, f0, t_start, n_periods, H):
    """t [n] accepted times of one instance (sample 0 = the arming point), v [n][P] the probe values there -> Ref with a, b [P][H+1]
    (mpf), their bounds da, db (float), the restated covered (double, the kernel's own operations) and the segments integrated"""
    t_end = t_start + float(n_periods) / f0  # (the host's doubles)
    ts, te = mp.mpf(t_start), mp.mpf(t_end)
    Tw = te - ts
    w0 = 2 * mp.pi * mp.mpf(f0)
    w0f = 2.0 * math.pi * f0
    K, P = H + 1, v.shape[1]
    C = [[mp.mpf(0)] * K for _ in range(P)]
    S = [[mp.mpf(0)] * K for _ in range(P)]
    bC, bS, aC, aS = (np.zeros((P, K)) for _ in range(4))
    ks = np.arange(K, dtype=float)
    k1 = ks > 0
    cov, nseg = 0.0, 0
    for i in range(1, len(t)):
        t0, t1 = float(t[i - 1]), float(t[i])
        if not (t1 > t_start) or not (t0 < t_end) or not (t1 > t0):
            continue
        nseg += 1
        clip_a, clip_b = t0 < t_start, t1 > t_end
        ta, tb = (t_start if clip_a else t0), (t_end if clip_b else t1)
        tau_a, tau_b = ta - t_start, tb - t_start
        h = tau_b - tau_a
        cov += h
        # ---- exact
        m0, m1, ma, mb = mp.mpf(t0), mp.mpf(t1), mp.mpf(ta), mp.mpf(tb)
        ra, rb = (ma - m0) / (m1 - m0), (mb - m0) / (m1 - m0)
        xa, xb = ma - ts, mb - ts
        hh = xb - xa
        ea = [mp.expj(-k * w0 * xa) for k in range(K)]
        eb = [mp.expj(-k * w0 * xb) for k in range(K)]
        # ---- bound: what depends on k alone
        tm = tau_a + 0.5 * h
        w = ks * w0f
        d_ta, d_tb = (U * abs(tau_a), U * abs(tau_b)) if t_start != 0.0 else (0.0, 0.0)
        d_h = d_ta + d_tb + U * h
        d_tm = d_ta + 0.5 * d_h + U * abs(tm)
        d_cs = np.where(k1, w * d_tm + 4 * U * np.abs(w * tm) + 2 * U, 0.0)
        phi = 0.5 * w * h
        d_phi = 0.5 * w * d_h + 4 * U * phi
        A, B = weights(phi)
        with np.errstate(all="ignore"):
            closed = np.where(np.abs(phi) >= SERIES_BELOW, 2 * U * (np.abs(phi * np.cos(phi)) + np.abs(np.sin(phi))) / np.where(phi != 0, 2 * phi * phi, 1.0), 0.0)
            dBdphi = np.where(phi != 0, np.abs(A / 2 - 2 * B / np.where(phi != 0, phi, 1.0)), 0.0)
        d_A = np.where(k1, 4 * U * np.abs(A) + 2 * np.abs(B) * d_phi, 0.0)
        d_B = np.where(k1, 4 * U * np.abs(B) + closed + dBdphi * d_phi, 0.0)
        cm, sm = np.cos(w * tm), np.sin(w * tm)
        for p in range(P):
            f0v, f1v = float(v[i - 1, p]), float(v[i, p])
            v0, v1 = mp.mpf(f0v), mp.mpf(f1v)
            va, vb = v0 + (v1 - v0) * ra, v0 + (v1 - v0) * rb
            beta = (vb - va) / hh
            C[p][0] += hh * (va + vb) / 2
            for k in range(1, K):
                wk = k * w0
                I = eb[k] * (mp.mpc(0, vb / wk) + beta / wk ** 2) - ea[k] * (mp.mpc(0, va / wk) + beta / wk ** 2)
                C[p][k] += I.real
                S[p][k] -= I.imag
            fa, fb = float(va), float(vb)
            d01 = abs(f1v - f0v)
            d_va = 4 * U * d01 + U * abs(fa) if clip_a else 0.0
            d_vb = 4 * U * d01 + U * abs(fb) if clip_b else 0.0
            vm, dd = 0.5 * (fa + fb), fb - fa
            d_vm = 0.5 * (d_va + d_vb) + U * abs(vm)
            d_dd = d_va + d_vb + U * abs(dd)
            pa, pb = vm * A, dd * B
            d_pa = np.abs(A) * d_vm + abs(vm) * d_A + U * np.abs(pa)
            d_pb = np.abs(B) * d_dd + abs(dd) * d_B + U * np.abs(pb)
            for (c1, s1, acc_b, acc_a, sign) in ((cm, sm, bC, aC, -1.0), (sm, cm, bS, aS, 1.0)):
                inner = pa * c1 + sign * pb * s1
                d_in = np.abs(c1) * d_pa + np.abs(s1) * d_pb + (np.abs(pa) + np.abs(pb)) * d_cs + U * np.abs(pb * s1) + U * np.abs(inner)
                c = h * inner
                acc_b[p] += np.abs(inner) * d_h + h * d_in + U * np.abs(c)
                acc_a[p] += np.abs(c)
    r = Ref()
    r.t_end, r.Tw, r.cov, r.nseg, r.H = t_end, Tw, cov, nseg, H
    Twf = float(Tw)
    scale = np.where(k1, 2.0, 1.0) / Twf
    r.a = [[(2 if k else 1) * C[p][k] / Tw for k in range(K)] for p in range(P)]
    r.b = [[(2 * S[p][k] / Tw if k else mp.mpf(0)) for k in range(K)] for p in range(P)]
    af = np.array([[float(x) for x in row] for row in r.a])
    bf = np.array([[float(x) for x in row] for row in r.b])
    Cf, Sf = af / scale, bf / scale
    r.da = scale * (bC + U * np.abs(Cf) + (nseg * U) ** 2 * aC) + 2 * U * np.abs(af)
    r.db = np.where(k1, scale * (bS + U * np.abs(Sf) + (nseg * U) ** 2 * aS) + 2 * U * np.abs(bf), 0.0)
    return r


def derived(r):
    """amp, phase, thd of the reference with the bounds propagated from a and b: (amp, d_amp, phase, d_phase [P][K]; thd, d_thd [P])"""
    P, K = len(r.a), r.H + 1
    amp = [[(mp.sqrt(r.a[p][k] ** 2 + r.b[p][k] ** 2) if k else abs(r.a[p][0])) for k in range(K)] for p in range(P)]
    ph = [[mp.atan2(-r.b[p][k] if k else mp.mpf(0), r.a[p][k]) for k in range(K)] for p in range(P)]
    af = np.array([[float(abs(x)) for x in row] for row in r.a])
    bf = np.array([[float(abs(x)) for x in row] for row in r.b])
    ampf = np.array([[float(x) for x in row] for row in amp])
    phf = np.array([[float(abs(x)) for x in row] for row in ph])
    with np.errstate(all="ignore"):
        d_amp = np.where(ampf > 0, (af * r.da + bf * r.db) / ampf, r.da + r.db) + 2 * U * ampf
        d_ph = np.where(ampf > 0, (af * r.db + bf * r.da) / ampf ** 2, np.inf) + 2 * U * phf
    d_amp[:, 0] = r.da[:, 0] + U * ampf[:, 0]
    thd, d_thd = [], []
    for p in range(P):
        s2 = sum((amp[p][k] ** 2 for k in range(2, K)), mp.mpf(0))
        th = mp.sqrt(s2) / amp[p][1]
        s2f, a1 = float(s2), ampf[p, 1]
        d_s2 = float(np.sum(2 * ampf[p, 2:] * d_amp[p, 2:])) + max(K - 3, 0) * U * s2f
        thf = float(th)
        d_thd.append((d_s2 / (2 * math.sqrt(s2f) * a1) if s2f > 0 else 0.0) + thf * d_amp[p, 1] / a1 + 2 * U * thf)
        thd.append(th)
    return amp, d_amp, ph, d_ph, thd, np.array(d_thd)


def compare(coef, thd, r, what, need_signal=True):
    """coef [P][K][4], thd [P] of one instance against the reference: -> worst |error| / bound (asserted <= 1)"""
    amp, d_amp, ph, d_ph, rthd, d_thd = derived(r)
    P, K = coef.shape[0], coef.shape[1]
    worst = 0.0
    for p in range(P):
        for k in range(K):
            for (got, ref, bound, name) in ((coef[p, k, 0], r.a[p][k], r.da[p, k], "a"), (coef[p, k, 1], r.b[p][k], r.db[p, k], "b"),
                                            (coef[p, k, 2], amp[p][k], d_amp[p, k], "amp")):
                err = float(abs(mp.mpf(float(got)) - ref))
                assert err <= bound, f"{what}: probe {p} {name}_{k} = {got!r}, reference {float(ref)!r}: error {err:.3g} > bound {bound:.3g}"
                if bound > 0:
                    worst = max(worst, err / bound)
            if math.isfinite(d_ph[p, k]) and float(amp[p][k]) >= 1000 * d_amp[p, k]:
                err = float(abs(mp.mpf(float(coef[p, k, 3])) - ph[p][k]))
                err = min(err, abs(err - 2 * math.pi))  # (the branch cut at +-pi)
                assert err <= d_ph[p, k], f"{what}: probe {p} phase_{k} = {coef[p, k, 3]!r}, reference {float(ph[p][k])!r}: error {err:.3g} > {d_ph[p, k]:.3g}"
                if d_ph[p, k] > 0:
                    worst = max(worst, err / d_ph[p, k])
        err = float(abs(mp.mpf(float(thd[p])) - rthd[p]))
        assert err <= d_thd[p], f"{what}: probe {p} thd = {thd[p]!r}, reference {float(rthd[p])!r}: error {err:.3g} > bound {d_thd[p]:.3g}"
        if d_thd[p] > 0:
            worst = max(worst, err / d_thd[p])
    if need_signal:
        a0 = np.array([float(x) for x in amp[0]])
        assert a0[1] >= 1000 * d_amp[0, 1], f"{what}: the fundamental {a0[1]:.3g} is within 1000 x its bound {d_amp[0, 1]:.3g}"
        assert K > 2 and np.any(a0[2:] >= 1000 * d_amp[0, 2:]), f"{what}: no harmonic k >= 2 above 1000 x its bound"
    return worst


def points(e, b=0):
    """accepted points of instance b of the armed window (needs stride 1 and room for all)"""
    t, v, n, drop = e.probe_samples()
    assert not drop.any(), drop
    return t[b, :n[b]].copy(), v[b, :n[b]].copy()


def configure(e, rows, four, capacity, stride=1, measures=()):
    e.set_probes(rows, capacity, stride, measures)
    if four is not None:
        e.set_fourier(**four)
    e.arm_probes()


def check_instance(e, b, four, what, need_signal=True):
    """instance b of an engine that holds every accepted point: coefficients, THD and covered against the reference; -> worst, Ref"""
    t, v = points(e, b)
    coef, thd, cov = e.fourier(b, 1)
    probes = list(four["probes"])
    first = [i for i, p in enumerate(probes) if probes.index(p) == i]  # (the rows of a duplicate are bit-equal: check_restatement)
    r = reference(t, v[:, [probes[i] for i in first]], four["f0"], four["t_start"], four["n_periods"], four["n_harmonics"])
    assert cov[0] == r.cov, f"{what}: covered {cov[0]!r}, restated {r.cov!r}"
    return compare(coef[0][first], thd[0][first], r, what, need_signal), r


# ---------------------------------------------------------------------------------------------------------------- 1. restatement
def four_of(name, H=9, probes=(0,), n_periods=2, t_start=0.0, f0=None):
    f0 = f0 or F0
    return dict(f0=f0, t_start=t_start, n_periods=n_periods, n_harmonics=H, probes=list(probes))


def check_restatement(name, knobs, label, H=9, probes=(0,), batch=1, adaptive=False, steps=64):
    """check 1: every coefficient, amp, phase and THD of every instance against the reference over the engine's own accepted points"""
    rows = DECKS[name][2]
    four = four_of(name, H, probes)
    e = engine(name, knobs, batch, AMPS3[:batch] if batch > 1 else None)
    if adaptive:
        configure(e, rows, four, 4096)
        st = e.analyze_tr_adaptive(2 * T0, T0 / 64, dt_max=T0 / 16, lte_reltol=1e-3, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0, source_breakpoints=True)
        assert st["rc"] == 0, st
    else:
        n = 2 * steps + 2  # (two steps past t_end: t is accumulated)
        configure(e, rows, four, n + 1)
        e.analyze_tr(T0 / steps, n)
    worst = 0.0
    coef, thd, cov = e.fourier()
    for b in range(batch):
        w, r = check_instance(e, b, four, f"{name} {label} instance {b}")
        worst = max(worst, w)
        assert abs(r.cov - float(r.Tw)) <= 4 * U * float(r.Tw) * 130, (r.cov, float(r.Tw))
        for i, p in enumerate(probes):  # a duplicate probe index gives bit-equal rows
            j = list(probes).index(p)
            assert same_bits(coef[b, i], coef[b, j]) and same_bits(thd[b, i], thd[b, j]), (b, i, j)
    if batch > 1 and name == "rectifier":
        assert len({float(x) for x in thd[:, 0]}) == batch, f"instances with different amplitudes have different THD: {thd[:, 0]}"
    e.close()
    print(f"FOURIER {label} worst {name} {'adaptive' if adaptive else 'fixed'} H {H} probes {len(probes)} batch {batch}: {worst:.3g}")
    return worst


def check_two_items(knobs, label):
    """H = 1 with one probe: two work items.  No harmonic k >= 2 exists, so the signal condition holds for the fundamental alone."""
    four = four_of("rectifier", 1, (0,))
    e = engine("rectifier", knobs)
    configure(e, DECKS["rectifier"][2], four, 131)
    e.analyze_tr(T0 / 64, 130)
    w, r = check_instance(e, 0, four, f"rectifier {label} H 1", need_signal=False)
    coef, thd, cov = e.fourier()
    amp, d_amp = derived(r)[:2]
    assert float(amp[0][1]) >= 1000 * d_amp[0, 1] and thd[0, 0] == 0.0, (thd, d_amp)
    e.close()
    print(f"FOURIER {label} worst rectifier H 1: {w:.3g}")


def check_compensation(knobs, label, periods=128):
    """the compensation term: 128 periods of pulse_src, 8192 steps, window from t = 0 (tau is then exact).  Against this bound the
    compensation can only show at k = 0: there the bound grows like 3 u sum |c_i| while a plain sum loses about u sum |partial sums|.
    For k >= 1 the sincos argument alone allows 4 u k w0 tau per term, which exceeds what a plain sum would lose: the bound cannot tell."""
    four = four_of("pulse_src", 1, (0,), n_periods=periods)
    n = 64 * periods + 2
    e = engine("pulse_src", knobs)
    configure(e, DECKS["pulse_src"][2], four, n + 1)
    e.analyze_tr(T0 / 64, n)
    w, r = check_instance(e, 0, four, f"pulse_src {label} {periods} periods", need_signal=False)
    e.close()
    print(f"FOURIER {label} worst pulse_src {periods} periods (compensated sum): {w:.3g}")


def check_tiny_steps(knobs, label):
    """the series arm of the weights: 200 steps of a ten-millionth of a period up the first rising edge of pulse_src, phi = k pi 1e-7.
    The closed form of B loses u / phi there, against a per-segment bound of a few u: the one case that tells the two arms apart below
    the threshold (above it, check 1 at 64 steps per period runs the closed arm at phi = k pi / 64 up to 3.1)."""
    four = four_of("pulse_src", 3, (0,), n_periods=1)
    e = engine("pulse_src", knobs)
    configure(e, DECKS["pulse_src"][2], four, 201)
    e.analyze_tr(T0 * 1e-7, 200)
    w, r = check_instance(e, 0, four, f"pulse_src {label} tiny steps", need_signal=False)
    assert 0 < r.cov < 1e-4 * T0 and float(r.a[0][1]) > 1e-10, (r.cov, float(r.a[0][1]))
    e.close()
    print(f"FOURIER {label} worst pulse_src tiny steps (series arm): {w:.3g}")


def check_batch_384(knobs, label):
    """vac_r at batch 384 (the resident kernels' 128-VGPR build): every instance is its own amplitude; three of them against the
    reference, all of them against amplitude scaling of the sampled sine to 1e-12"""
    B, four = 384, four_of("vac_r", 20)
    amps = [1.0 + 0.001 * b for b in range(B)]
    e = engine("vac_r", knobs, B, amps)
    configure(e, DECKS["vac_r"][2], four, 35)
    e.analyze_tr(T0 / 16, 34)
    coef, thd, cov = e.fourier()
    worst = max(check_instance(e, b, four, f"vac_r {label} batch 384 instance {b}")[0] for b in (0, 191, 383))
    assert np.all(cov == cov[0]) and np.allclose(coef[:, 0, 1, 2], np.array(amps) * coef[0, 0, 1, 2], rtol=1e-12, atol=0)
    e.close()
    print(f"FOURIER {label} worst vac_r batch 384: {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------- 2. closed forms
def trapezoid(tt, amp=1.0):
    """the ideal PULSE of pulse_src at time tt (mpf): period 1 / F0, edges of a period / 8, on for half of it"""
    T = 1 / mp.mpf(F0)
    x = tt - mp.floor(tt / T) * T
    e = T / 8
    if x < e:
        return amp * x / e
    if x < T / 2 - e:
        return mp.mpf(amp)
    if x < T / 2:
        return amp * (T / 2 - x) / e
    return mp.mpf(0)


def closed_allowance(t, v, r, ideal, t_dev=None, slope=0.0):
    """(2 / Tw) sum h (max |v_sample - ideal(t_sample)| + slope max |t_sample - t_grid|) over the segments that touch the window, plus
    the part of the window the accepted steps did not cover at the largest |v|: what the recorded run itself is away from the ideal wave"""
    dev = [float(abs(mp.mpf(float(v[i])) - ideal(i, mp.mpf(float(t[i]))))) for i in range(len(t))]
    td = [0.0] * len(t) if t_dev is None else t_dev
    s = 0.0
    for i in range(1, len(t)):
        if t[i] > float(r.t_end) - float(r.Tw) and t[i - 1] < r.t_end:
            s += (t[i] - t[i - 1]) * (max(dev[i - 1], dev[i]) + slope * max(td[i - 1], td[i]))
    s += abs(float(r.Tw) - r.cov) * float(np.max(np.abs(v)))
    return 2.0 / float(r.Tw) * s


def check_closed_pulse(knobs, label):
    """check 2a: pulse_src under the adaptive transient with the generator's corners as breakpoints: the node voltage is piecewise linear
    between the corners, so the exact integral of the interpolant is the Fourier series of the trapezoid wave, whatever steps were taken"""
    H = 21
    T = 1 / mp.mpf(F0)
    worst = 0.0
    for case, four, t_stop in (("periods", four_of("pulse_src", H), 2 * T0),
                               ("clipped", four_of("pulse_src", H, n_periods=1, t_start=T0 / 16, f0=1.0 / (0.375 * T0)), T0)):
        e = engine("pulse_src", knobs)
        configure(e, DECKS["pulse_src"][2], four, 4096)
        st = e.analyze_tr_adaptive(t_stop, T0 / 64, dt_max=T0 / 8, source_breakpoints=True)
        assert st["rc"] == 0, st
        t, v = points(e)
        coef, thd, cov = e.fourier()
        r = reference(t, v[:, [0]], four["f0"], four["t_start"], four["n_periods"], H)
        allow = closed_allowance(t, v[:, 0], r, lambda i, tt: trapezoid(tt))
        assert allow < 1e-12, f"the recorded run is {allow:.3g} away from the ideal trapezoid: the deck is wrong, not the cap"
        ts, te = mp.mpf(four["t_start"]), mp.mpf(r.t_end)
        for k in range(H + 1):
            if case == "periods":
                if k == 0:
                    z = mp.mpf(3) / 8
                else:  # a continuous piecewise-linear periodic wave: int f e^{-jwt} dt = -(1 / w^2) sum (slope after - slope before) e^{-jw t_i}
                    w = 2 * mp.pi * F0 * k
                    jumps = ((0, 8 / T), (T / 8, -8 / T), (3 * T / 8, -8 / T), (T / 2, 8 / T))
                    z = 2 / T * (-1 / w ** 2) * sum(ds * mp.expj(-w * ti) for ti, ds in jumps)
            else:
                w = 2 * mp.pi * mp.mpf(four["f0"]) * k
                cuts = [ts] + [c for c in (T / 8, 3 * T / 8) if ts < c < te] + [te]
                z = sum(mp.quad(lambda x: trapezoid(x) * mp.expj(-w * (x - ts)), [cuts[i], cuts[i + 1]]) for i in range(len(cuts) - 1)) * (2 if k else 1) / (te - ts)
            for got, ref, bound, nm in ((coef[0, 0, k, 0], mp.re(z), r.da[0, k], "a"), (coef[0, 0, k, 1], -mp.im(z) if k else mp.mpf(0), r.db[0, k], "b")):
                err = float(abs(mp.mpf(float(got)) - ref))
                assert err <= bound + allow, f"pulse_src {case} {nm}_{k} = {got!r}, closed form {float(ref)!r}: error {err:.3g} > {bound:.3g} + {allow:.3g}"
                worst = max(worst, err / (bound + allow))
        e.close()
    print(f"FOURIER {label} worst pulse_src closed form: {worst:.3g} (allowance of the run {allow:.3g})")


def check_closed_sine(knobs, label):
    """check 2b: vac_r with 16 uniform steps per period: the interpolant of a sampled sine has b_k = +-A sinc^2(pi k / 16) at k = 1, 15,
    17 (the aliases of the fundamental) and nothing else"""
    H, N = 20, 16
    four = four_of("vac_r", H)
    e = engine("vac_r", knobs)
    configure(e, DECKS["vac_r"][2], four, 2 * N + 3)
    e.analyze_tr(T0 / N, 2 * N + 2)
    t, v = points(e)
    coef, thd, cov = e.fourier()
    r = reference(t, v[:, [0]], F0, 0.0, 2, H)
    grid = [mp.mpf(i) / (N * mp.mpf(F0)) for i in range(len(t))]
    t_dev = [float(abs(mp.mpf(float(t[i])) - grid[i])) for i in range(len(t))]
    allow = closed_allowance(t, v[:, 0], r, lambda i, tt: mp.sin(2 * mp.pi * F0 * grid[i]), t_dev, 2 * math.pi * F0)
    assert allow < 1e-12, allow
    worst = 0.0
    for k in range(H + 1):
        x = mp.pi * k / N
        bk = {1: 1, 15: -1, 17: 1}.get(k, 0) * ((mp.sin(x) / x) ** 2 if k else 0)
        for got, ref, bound, nm in ((coef[0, 0, k, 0], mp.mpf(0), r.da[0, k], "a"), (coef[0, 0, k, 1], bk, r.db[0, k], "b")):
            err = float(abs(mp.mpf(float(got)) - ref))
            assert err <= bound + allow, f"vac_r {nm}_{k} = {got!r}, closed form {float(ref)!r}: error {err:.3g} > {bound:.3g} + {allow:.3g}"
            worst = max(worst, err / (bound + allow))
    e.close()
    print(f"FOURIER {label} worst vac_r closed form: {worst:.3g} (allowance of the run {allow:.3g})")


# ---------------------------------------------------------------------------------------------------------------- 3. + 4. independence
MEAS = [("min", 0), ("max", 0), ("avg", 1), ("rms", 0), ("integ", 1), ("cross", 0, 0.5, 1, 1)]


def check_sample_buffer(knobs, label):
    """check 3: stride and capacity of the sample buffer do not reach the accumulation, and the accumulation does not reach them"""
    rows, four, n = DECKS["rectifier"][2], four_of("rectifier", 9, (0, 1)), 130
    out = {}
    for key, f4, cap, stride in (("full", four, n + 1, 1), ("thin", four, 1, 7), ("none", None, n + 1, 1)):
        e = engine("rectifier", knobs)
        configure(e, rows, f4, cap, stride, MEAS)
        e.analyze_tr(T0 / 64, n)
        out[key] = (e.fourier() if f4 else None, e.probe_samples(), e.measures(), e.solution())
        e.close()
    for a, b in zip(out["full"][0], out["thin"][0]):
        assert same_bits(a, b), "stride 7 / capacity 1 changes the coefficients"
    assert out["thin"][1][2][0] == 1 and out["thin"][1][3][0] == n // 7
    for a, b in zip(out["full"][1:], out["none"][1:]):
        for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
            assert same_bits(x, y), "samples, measures or the solution differ once a Fourier analysis is configured"
    assert same_bits(out["full"][2], out["thin"][2]), "measures"
    print(f"FOURIER {label} sample buffer independent")


def check_batch(knobs, label):
    """check 4: each instance of a batch of 3 is bit-identical to its own batch-1 run (fixed steps), and the THDs differ"""
    rows, four, n = DECKS["rectifier"][2], four_of("rectifier", 9, (0, 1)), 130
    e = engine("rectifier", knobs, 3, AMPS3)
    configure(e, rows, four, 1)
    e.analyze_tr(T0 / 64, n)
    c3, t3, v3 = e.fourier()
    e.close()
    for b in range(3):
        e = engine("rectifier", knobs, 1, AMPS3[b:b + 1])
        configure(e, rows, four, 1)
        e.analyze_tr(T0 / 64, n)
        c1, t1, v1 = e.fourier()
        e.close()
        assert same_bits(c3[b], c1[0]) and same_bits(t3[b], t1[0]) and same_bits(v3[b], v1[0]), f"instance {b} of the batch differs from its own run"
    assert len({float(x) for x in t3[:, 0]}) == 3, t3
    print(f"FOURIER {label} batch of 3 bit-identical to single runs, thd {t3[:, 0]}")


# ---------------------------------------------------------------------------------------------------------------- 5. window rules
def check_window_rules(knobs, label):
    rows, dt = DECKS["rectifier"][2], T0 / 64
    four = four_of("rectifier", 9, (0,), n_periods=1, t_start=T0)
    nan3 = lambda r: all(np.all(np.isnan(x)) for x in r[:2])
    # not armed, then a window not yet reached: covered 0, NaN
    e = engine("rectifier", knobs)
    e.set_probes(rows, 300)
    e.set_fourier(**four)
    r = e.fourier()
    assert nan3(r) and r[2][0] == 0.0, r
    e.arm_probes()
    e.analyze_tr(dt, 40)
    r = e.fourier()
    assert nan3(r) and r[2][0] == 0.0, r
    # split calls equal one call; steps beyond t_end change nothing once a step has ended at or beyond it
    e.analyze_tr(dt, 60)
    e.analyze_tr(dt, 32)
    assert e.state()["t"][0] >= 2 * T0
    split = e.fourier()
    w, ref = check_instance(e, 0, four, f"rectifier {label} window one period in")
    e.analyze_tr(dt, 9)
    assert all(same_bits(a, b) for a, b in zip(split, e.fourier())), "steps past t_end changed the result"
    f = engine("rectifier", knobs)
    configure(f, rows, four, 300)
    f.analyze_tr(dt, 132)
    assert all(same_bits(a, b) for a, b in zip(split, f.fourier())), "analyze_tr(dt, n1), (dt, n2), (dt, n3) differs from one call"
    # arming after t_start: covered < Tw, exactly the restated clipped length (check_instance), NaN no more
    g = engine("rectifier", knobs)
    g.analyze_tr(dt, 80)
    configure(g, rows, four, 300)
    g.analyze_tr(dt, 60)
    check_instance(g, 0, four, f"rectifier {label} armed late", need_signal=False)
    cov = g.fourier()[2][0]
    assert 0 < cov < T0 * (1 - 1e-3) and abs(cov - (2 * T0 - 80 * dt)) < 1e-9 * T0, cov
    # everything that disarms: what was accumulated stays readable and no longer moves; arming again zeroes
    blob = f.checkpoint()
    x = f.solution()
    for how in ("analyze_dc", "reset", "set_solution", "set_time", "checkpoint_load"):
        h = engine("rectifier", knobs)
        configure(h, rows, four, 300)
        h.analyze_tr(dt, 100)
        before = h.fourier()
        if how == "analyze_dc":
            h.analyze_dc(F.MODE_TROP)
        elif how == "reset":
            h.reset()
        elif how == "set_solution":
            h.set_solution(x)
        elif how == "set_time":
            lib = F.lib()
            assert lib.pe_hip_set_time(h._h, F.C.c_double(100 * dt), F.C.c_double(dt)) == 0
        else:
            h.restore(blob)
        assert all(same_bits(a, b) for a, b in zip(before, h.fourier())), how
        h.analyze_tr(dt, 5)
        assert all(same_bits(a, b) for a, b in zip(before, h.fourier())), f"{how} did not disarm"
        h.arm_probes()
        r = h.fourier()
        assert nan3(r) and r[2][0] == 0.0, f"arming after {how} did not zero the accumulators"
        h.close()
    for q in (e, f, g):
        q.close()
    print(f"FOURIER {label} worst rectifier window rules: {w:.3g}")


# ---------------------------------------------------------------------------------------------------------------- 6. adaptive transient
def check_adaptive_rejections(knobs, label):
    """check 6: step logs with rejected steps of both kinds; the coefficients are the reference over the accepted points only and the
    segments integrated are the accepted steps.  pulse_rc is linear, so Newton never fails on it and its log holds LTE rejections only;
    the rectifier with a Newton cap of 5 (as in the tests of the adaptive transient) adds the Newton rejections."""
    worst = 0.0
    for name, opt, need in (("pulse_rc", {}, ("n_rejected_lte",)), ("rectifier", {"max_newton": 3}, ("n_rejected_lte", "n_rejected_newton"))):
        four = four_of(name, 9, (0,))
        e = engine(name, knobs, **opt)
        configure(e, DECKS[name][2], four, 8192)
        st = e.analyze_tr_adaptive(2 * T0, T0 / 20, lte_reltol=1e-3, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0, source_breakpoints=True)
        assert st["rc"] == 0 and all(st[k] > 0 for k in need), st
        t, v = points(e)
        w, r = check_instance(e, 0, four, f"{name} {label} adaptive with rejections")
        assert r.nseg == st["n_accepted"] == len(t) - 1, (r.nseg, st["n_accepted"], len(t))
        worst = max(worst, w)
        print(f"FOURIER {label} {name}: accepted {st['n_accepted']} rejected lte {st['n_rejected_lte']} newton {st['n_rejected_newton']}")
        e.close()
    print(f"FOURIER {label} worst adaptive with rejections: {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def check_refusals(knobs, label):
    lib, C = F.lib(), F.C
    rows, n = DECKS["rectifier"][2], 130
    e = F.Engine()
    one, two, neg = (np.array(a, dtype=np.int32) for a in ([0], [0, 3], [-1]))  # (kept alive: the controls point into them)

    def ctl(**kw):
        c = dict(dict(f0=F0, t_start=0.0, n_periods=2, n_harmonics=9, n_probes=1, probes=F._ip(one)), **kw)
        return F.FourierControl(*[c[k] for k in ("f0", "t_start", "n_periods", "n_harmonics", "n_probes", "probes")])

    assert lib.pe_hip_set_fourier(e._h, C.byref(ctl())) == F.ERR_ARG, "no circuit"
    e.close()
    e = engine("rectifier", knobs)
    assert lib.pe_hip_set_fourier(e._h, C.byref(ctl())) == F.ERR_ARG, "no probes"
    assert lib.pe_hip_get_fourier(e._h, 0, 1, None, None, None) == F.ERR_ARG
    configure(e, rows, four_of("rectifier", 9, (0, 1)), 1)
    e.analyze_tr(T0 / 64, n)
    good = e.fourier()
    bad = [dict(f0=0.0), dict(f0=-1.0), dict(f0=math.nan), dict(f0=math.inf), dict(t_start=math.nan), dict(t_start=-math.inf), dict(n_periods=0),
           dict(n_harmonics=0), dict(n_harmonics=64), dict(n_probes=-1), dict(n_probes=2, probes=F._ip(two)),
           dict(probes=F._ip(neg)), dict(f0=5e-324),
           dict(t_start=1e300, f0=1e3)]  # (1 / 5e-324 overflows: t_end not finite; 1e300 + 2e-3 == 1e300: t_end not > t_start)
    for kw in bad:
        assert lib.pe_hip_set_fourier(e._h, C.byref(ctl(**kw))) == F.ERR_ARG, kw
        assert all(same_bits(a, b) for a, b in zip(good, e.fourier())), f"a refused configuration changed the result: {kw}"
    assert lib.pe_hip_get_fourier(e._h, 0, 2, None, None, None) == F.ERR_ARG and lib.pe_hip_get_fourier(e._h, -1, 1, None, None, None) == F.ERR_ARG
    # ... and the engine goes on as if nothing had been asked: the window is still armed
    e.analyze_tr(T0 / 64, 4)
    f = engine("rectifier", knobs)
    configure(f, rows, four_of("rectifier", 9, (0, 1)), 1)
    f.analyze_tr(T0 / 64, n + 4)
    assert all(same_bits(a, b) for a, b in zip(f.fourier(), e.fourier()))
    # a successful call ends the window like pe_hip_set_probes; NULL removes the analysis; set_probes drops it
    e.set_fourier(**four_of("rectifier", 3, (1,)))
    e.analyze_tr(T0 / 64, 4)
    r = e.fourier()
    assert r[0].shape == (1, 1, 4, 4) and np.all(np.isnan(r[0])) and r[2][0] == 0.0
    e.set_fourier()
    assert lib.pe_hip_get_fourier(e._h, 0, 1, None, None, None) == F.ERR_ARG
    e.set_fourier(**four_of("rectifier", 3, (1,)))
    e.set_probes(rows, 4)
    assert lib.pe_hip_get_fourier(e._h, 0, 1, None, None, None) == F.ERR_ARG
    e.arm_probes()
    e.analyze_tr(T0 / 64, 3)
    e.close()
    f.close()
    print(f"FOURIER {label} refusals")


# ---------------------------------------------------------------------------------------------------------------- 8. sweep handle
def check_sweep(label):
    """two (emulated) devices against one engine: identical bits per instance"""
    B, n = 5, 130
    deck, gmin, rows, par, a0 = DECKS["rectifier"]
    amps = np.array([a0 * (0.5 + 0.25 * b) for b in range(B)])
    ov = {"VAC": np.stack([amps, np.full(B, 2.0 * math.pi * F0), np.zeros(B)], 1)[:, None, :]}
    four = four_of("rectifier", 9, (0, 1))
    e = F.Engine()
    e.set_options(g_min=gmin)
    e.load_deck(deck(), B, ov)
    e.reset()
    configure(e, rows, four, 1)
    e.analyze_tr(T0 / 64, n)
    one = e.fourier()
    e.close()
    s = F.Sweep(device_mask=3)
    assert len(s.shards()) == 2, s.shards()
    s.set_options(g_min=gmin)
    s.load_deck(deck(), B, ov)
    s.reset()
    configure(s, rows, four, 1)
    s.run(T0 / 64, n)
    assert all(same_bits(a, b) for a, b in zip(one, s.fourier()))
    assert all(same_bits(a[1:4], b) for a, b in zip(one, s.fourier(1, 3))), "a range across the two devices"
    lib = F.lib()
    assert lib.pe_hip_sweep_get_fourier(s._h, 0, B + 1, None, None, None) == F.ERR_ARG
    s.set_fourier()
    assert lib.pe_hip_sweep_get_fourier(s._h, 0, 1, None, None, None) == F.ERR_ARG
    s.close()
    print(f"FOURIER {label} sweep over two devices bit-identical, thd {one[1][:, 0]}")


# ---------------------------------------------------------------------------------------------------------------- 9. values for the C++ test
def cpp_expectations(knobs, label):
    """what tests/cpp/fourier_rectifier.cpp must find: THD of v(k) of `rectifier` (2 periods of 64 steps + 2, H = 9) from the reference
    over this library's own run, with its propagated bound"""
    four = four_of("rectifier", 9, (0,))
    e = engine("rectifier", knobs)
    configure(e, DECKS["rectifier"][2], four, 131)
    e.analyze_tr(T0 / 64, 130)
    t, v = points(e)
    r = reference(t, v[:, [0]], F0, 0.0, 2, 9)
    amp, d_amp, ph, d_ph, thd, d_thd = derived(r)
    e.close()
    return float(thd[0]), float(d_thd[0])
