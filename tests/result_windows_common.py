"""The window check of the stored-result getters at its edges (tests/test_result_windows_emu.py on the host emulation,
tests/test_gpu_result_windows.py on the device): pe_hip_get_ac_sweep, pe_hip_get_noise, pe_hip_get_noise_source_density,
pe_hip_get_noise_integrated, pe_hip_get_sens, pe_hip_get_net, pe_hip_get_net_status, pe_hip_get_dc_sweep and pe_hip_get_dc_sweep_status
(include/pe_hip.h).

Circuit.  VAC 1 V - R - (C || D) to ground at batch 2 (the instances differ in R); 3 frequency points, 2 outputs, 2 ports, 3 DC-sweep values
and the kept rows [1, 0] on both sweeps: the smallest sizes at which points, instances and kept rows are each more than one and different
from each other.  One port sits on the node the source holds, so the admittance matrices do not exist: NaN planes and a non-zero status.

Windows.  (first, n) over the points (outputs) and (first_instance, count) over the instances each take WINDOWS(all); every combination is
called with output buffers of the full size, pre-filled with a sentinel.  Both pairs inside: PE_HIP_OK, the first n x count blocks of every
buffer equal the slice of the full read byte for byte (NaN compares equal to itself that way) and the rest still holds the sentinel -- an
empty window writes nothing.  Either pair outside: PE_HIP_ERR_ARG, "out of range" in the message, every sentinel in place.

Every case is a function of (pe, knobs): the emulation test runs it in a child process, the GPU test in its own."""
import numpy as np

INT_MAX = 2 ** 31 - 1
W3 = [1e2, 1e3, 1e5]
PORTS = [(0, -1), (1, -1)]
OUTPUTS = [1, 0]
KEPT = [1, 0]
DC_VALUES = [500.0, 1000.0, 2000.0]
SENTINEL = {np.dtype(np.float64): np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.float64)[0],
            np.dtype(np.int32): np.int32(0x5A5A5A5A)}


def windows(n_all):
    """(first, n, inside)"""
    return [(0, n_all, True), (n_all, 0, True), (1, n_all - 1, True),
            (n_all, 1, False), (0, n_all + 1, False), (-1, 1, False), (0, -1, False), (INT_MAX, 1, False), (1, INT_MAX, False)]


def deck(pe):
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VAC", (1, 0), 1.0, 1000.0, 0.0)
    d.add("R", (1, 2), 1000.0)
    d.add("C", (2, 0), 1e-6)
    d.add("D", (2, 0))
    return d


def engine(pe, knobs=None):
    """the circuit at batch 2 after one call of each of the five analyses"""
    F = pe.ffi
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        if v is not None:
            e.set_knob(k, v)
    e.load_deck(deck(pe), 2, {"R": np.array([[[1000.0]], [[2200.0]]])})
    e.reset()
    e.analyze_dc(F.MODE_OP)
    e.set_ac_sweep_rows(KEPT)
    e.analyze_ac_sweep(W3)
    e.analyze_noise(W3, 1, contributions=True)
    n_par = len(e.sens_params()["kind"])
    e.analyze_sens(OUTPUTS, weight=np.linspace(1.0, 2.0, n_par), keep=True)
    e.analyze_net(W3, PORTS)
    e.set_dc_sweep_rows(KEPT)
    e.analyze_dc_sweep(DC_VALUES, F.R, 0)
    return e


def getters(pe, e):
    """name -> (items: points / outputs of the stored result, None for a per-instance getter; [(dtype, values per (item, instance))] of
    its output buffers; call(first, n, first_instance, count, pointers) -> status; its "no ... yet" text)"""
    F = pe.ffi
    lib, h = F.lib(), e._h
    n_src, n_par = len(e.noise_sources()["kind"]), len(e.sens_params()["kind"])
    assert n_src > 1 and n_par > 1, (n_src, n_par)
    f8, i4 = np.dtype(np.float64), np.dtype(np.int32)
    nn = len(PORTS) ** 2
    G = {
        "get_ac_sweep": (len(W3), [(f8, len(KEPT))] * 2, lambda a, n, b, c, p: lib.pe_hip_get_ac_sweep(h, a, n, b, c, *p), b"no AC sweep yet"),
        "get_noise": (len(W3), [(f8, 1), (f8, n_src)], lambda a, n, b, c, p: lib.pe_hip_get_noise(h, a, n, b, c, *p), b"no noise analysis yet"),
        "get_noise_source_density": (None, [(f8, n_src)], lambda a, n, b, c, p: lib.pe_hip_get_noise_source_density(h, b, c, *p), b"no noise analysis yet"),
        "get_noise_integrated": (None, [(f8, 1)], lambda a, n, b, c, p: lib.pe_hip_get_noise_integrated(h, b, c, *p), b"no noise analysis yet"),
        "get_sens": (len(OUTPUTS), [(f8, n_par), (f8, 1)], lambda a, n, b, c, p: lib.pe_hip_get_sens(h, a, n, b, c, *p), b"no sensitivity analysis yet"),
        "get_net_status": (len(W3), [(i4, 1)] * 2, lambda a, n, b, c, p: lib.pe_hip_get_net_status(h, a, n, b, c, *p), b"no network analysis yet"),
        "get_dc_sweep": (len(DC_VALUES), [(f8, len(KEPT))], lambda a, n, b, c, p: lib.pe_hip_get_dc_sweep(h, a, n, b, c, *p), b"no DC sweep yet"),
        "get_dc_sweep_status": (len(DC_VALUES), [(i4, 1)] * 3, lambda a, n, b, c, p: lib.pe_hip_get_dc_sweep_status(h, a, n, b, c, *p), b"no DC sweep yet"),
    }
    for which, tag in ((F.NET_Z, "Z"), (F.NET_Y, "Y"), (F.NET_S, "S")):
        G["get_net " + tag] = (len(W3), [(f8, nn)] * 2, lambda a, n, b, c, p, which=which: lib.pe_hip_get_net(h, which, a, n, b, c, *p), b"no network analysis yet")
    return G


def _buffers(F, items, outs, B):
    bufs = [np.full((items or 1) * B * w, SENTINEL[dt], dtype=dt) for dt, w in outs]
    return bufs, [F._dp(b) if b.dtype == np.float64 else F._ip(b) for b in bufs]


def check_windows(pe, knobs=None):
    F = pe.ffi
    lib = F.lib()
    e = engine(pe, knobs)
    try:
        B = e.batch
        n_calls = 0
        for name, (items, outs, call, _) in getters(pe, e).items():
            full, ptrs = _buffers(F, items, outs, B)
            assert call(0, items or 1, 0, B, ptrs) == 0, (name, lib.pe_hip_last_error(e._h))
            full = [f.reshape(items or 1, B, w) for f, (_, w) in zip(full, outs)]
            for f in full:
                bits = np.dtype("u%d" % f.itemsize)
                assert not np.any(f.view(bits) == SENTINEL[f.dtype].view(bits)), (name, "the full read writes every element")
            if name == "get_net Y":
                assert all(np.all(np.isnan(f)) for f in full), "a port on the held node: Y does not exist"
            if name == "get_net_status":
                assert np.all(full[0] == F.ERR_SINGULAR) and not full[1].any(), full
            for first, n, in_p in (windows(items) if items else [(0, 1, True)]):
                for fi, cnt, in_i in windows(B):
                    bufs, ptrs = _buffers(F, items, outs, B)
                    rc = call(first, n, fi, cnt, ptrs)
                    n_calls += 1
                    what = (name, first, n, fi, cnt)
                    if in_p and in_i:
                        assert rc == 0, (what, rc, lib.pe_hip_last_error(e._h))
                        for buf, f, (dt, w) in zip(bufs, full, outs):
                            want = np.ascontiguousarray(f[first:first + n, fi:fi + cnt]).tobytes()
                            got = buf.tobytes()
                            assert len(want) == n * cnt * w * dt.itemsize and got[:len(want)] == want, (what, "the window differs from the slice of the full read")
                            assert got[len(want):] == SENTINEL[dt].tobytes() * (len(buf) - n * cnt * w), (what, "written past the window")
                    else:
                        msg = lib.pe_hip_last_error(e._h)
                        assert rc == F.ERR_ARG and b"out of range" in msg and name.split()[0].encode() + b":" in msg, (what, rc, msg)
                        for buf, (dt, w) in zip(bufs, outs):
                            assert buf.tobytes() == SENTINEL[dt].tobytes() * len(buf), (what, "a refused call wrote")
        print("result windows:", n_calls, "calls")
    finally:
        e.close()


def check_validity(pe, knobs=None):
    F = pe.ffi
    lib = F.lib()
    e = engine(pe, knobs)
    try:
        B = e.batch
        G = getters(pe, e)

        def answer(name):
            items, outs, call, text = G[name]
            bufs, ptrs = _buffers(F, items, outs, B)
            rc = call(0, items or 1, 0, B, ptrs)
            return rc, lib.pe_hip_last_error(e._h), text, all(b.tobytes() == SENTINEL[b.dtype].tobytes() * len(b) for b in bufs)
        for name in G:
            assert answer(name)[0] == 0, name
        e.update_param(F.R, 0, 0, 1234.0)
        for name in G:
            rc, msg, text, untouched = answer(name)
            if name.startswith("get_dc_sweep"):
                continue
            assert rc == F.ERR_ARG and text in msg and name.split()[0].encode() + b":" in msg and untouched, (name, rc, msg)
        e.analyze_dc_sweep(DC_VALUES, F.R, 0)
        for name in ("get_dc_sweep", "get_dc_sweep_status"):
            assert answer(name)[0] == 0, name
        e.set_dc_sweep_rows(None)
        for name in ("get_dc_sweep", "get_dc_sweep_status"):
            rc, msg, text, untouched = answer(name)
            assert rc == F.ERR_ARG and text in msg and name.encode() + b":" in msg and untouched, (name, rc, msg)
    finally:
        e.close()
