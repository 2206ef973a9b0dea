#!/usr/bin/env python3
"""Fixtures of the pole-zero tests whose mpmath truth is too slow for a test (tests/pz_common.py reads them):

  tests/golden/pz_mesh16_poles.json   the 40 poles nearest to s0 = j 1e8 of rc_mesh(16, 16, seed, True), seeds 1 and 2 (258 complex rows),
                                      with their condition numbers: eigenvalues of A0^-1 (omega0 B) at 50 digits, condition numbers in binary64
  tests/golden/pz_mesh6_truth.json    poles and zeros (ports (1, -1) -> (30, 17)) of rc_mesh(6, 6, seed, True), seeds 1 .. 3, at s0 = j 1e9, keyed by a
                                      hash of G, B, the shift and the ports
  tests/golden/pz_eig_truth.json      eigenvalues, condition numbers and last eigenvector components of the matrices of pz_common.eig_matrices()
                                      at 50 digits, keyed by a hash of each matrix's bytes

Also prints the two measured constants of tests/pz_common.py again: E_MEASURED (the float64 restatement on the parity cases) and
C_LAPACK_MEASURED (numpy.linalg.eigvals on the matrices of the dense-solver test).  Needs no GPU: python scripts/pz_make_golden.py [mesh6] [mesh] [eig] [constants]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import pe_load  # noqa: E402

pe = pe_load.load()
O = pe_load.load_oracle()
import net_common as N  # noqa: E402
import pz_common as P  # noqa: E402

what = sys.argv[1:] or ["mesh6", "mesh", "eig", "constants"]
if "mesh6" in what:
    out = {}
    for seed in (1, 2, 3):
        G, B = P.pencil(N.oracle(O, pe.deck.rc_mesh(6, 6, seed, True)))
        for ports in (None, P.MESH6_PORTS):
            s, k = P.truth(G, B, P.MESH6_W0, ports)
            out[P.truth_key(G, B, P.MESH6_W0, ports)] = {"name": "rc_mesh(6, 6, %d, True) %s" % (seed, "zeros" if ports else "poles"),
                                                         "s": [[float(v.real), float(v.imag)] for v in s], "kappa": [float(min(v, 1e300)) for v in k]}
    with open(P.GOLDEN_TRUTH, "w") as f:
        json.dump(out, f, indent=0)
if "mesh" in what:
    out = {"omega0": P.MESH16_W0, "seeds": P.MESH16_SEEDS, "poles": [], "kappa": []}
    for seed in P.MESH16_SEEDS:
        G, B = P.pencil(N.oracle(O, pe.deck.rc_mesh(16, 16, seed, True)))
        # (mpmath's eigenvalues take ten minutes per instance at this size, its eigenvectors twice that again: the condition numbers, of
        # which a bound needs two digits, come from scipy's eigenvectors in binary64 -- they are 1.00x on this mesh)
        s, _ = P.truth(G, B, P.MESH16_W0, kappa=False, stable=False)   # (poles: the pencil itself has no defective infinite eigenvalue)
        k = P.kappa_float64(G, B, P.MESH16_W0, s[:40])
        print("seed", seed, "finite poles", len(s), "nearest", s[:3], flush=True)
        out["poles"].append([[float(v.real), float(v.imag)] for v in s[:40]])
        out["kappa"].append([float(v) for v in k])
    out["method"] = "eigenvalues: mpmath at 50 digits; condition numbers: scipy left and right eigenvectors in binary64"
    with open(P.GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
if "eig" in what:
    out = {}
    for name, Hs in P.eig_matrices().items():
        for i, H in enumerate(Hs):
            if not P.eig_checked(len(Hs), i):
                continue
            th, kap, last = P._eig_truth(H)
            out[P.eig_key(H)] = {"name": "%s [%d]" % (name, i), "theta": [[float(t.real), float(t.imag)] for t in th],
                                 "kappa": [float(min(k, 1e300)) for k in kap], "last": [float(v) for v in last]}
        print(name, "done", flush=True)
    with open(P.GOLDEN_EIG, "w") as f:
        json.dump(out, f, indent=0)
if "constants" in what:
    P.measure_e(pe, O)
    P.eig_cases(None)
