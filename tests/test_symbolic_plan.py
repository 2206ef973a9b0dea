"""CPU: the plans of the symbolic analysis, pinned bit for bit.  tests/cpp/symbolic_plan.cpp analyses a corpus of patterns under the
option sets the engine's policy uses and prints, per case, the outcome and one FNV-1a-64 hash per group of Symbolic's fields (permutations,
front tables, own entries, static, schedule, storage, child maps, quad plan, assembly lists); the program itself checks that every case
takes the path it is there for.  pe_symbolic.cpp is pure host C++, so the program is built from it alone, twice -- plainly at -O2 and
under AddressSanitizer + UBSan, both ordinary executables -- and every line of both must equal tests/golden/symbolic_plans.json.

The fixture records what the analysis computed BEFORE it was cut into phases: it was written by this program built against the sources
of the commit before that change,
    git worktree add <dir> <that commit>
    make -B -C tests/cpp symplan SYMPLAN_CSRC=<dir>/phy-engine_amd/csrc && tests/cpp/_build/symbolic_plan
and is regenerated the same way -- from the commit BEFORE a change that means to alter no plan, never from the changed code."""
import json
import os
import subprocess

import pytest

from parity_common import ROOT, make

CPP = os.path.join(ROOT, "tests", "cpp")


def expected_lines():
    with open(os.path.join(ROOT, "tests", "golden", "symbolic_plans.json")) as f:
        return json.load(f)["lines"]


@pytest.mark.parametrize("target, path", [("symplan", "_build/symbolic_plan"), ("symplan_san", "_build_asan/symbolic_plan")])
def test_symbolic_plans_match_the_fixture(target, path):
    make("-C", CPP, target)
    out = subprocess.run([os.path.join(CPP, path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"symbolic_plan ({target}) exited {out.returncode}: {out.stderr}"
    assert out.stderr == "", out.stderr  # (a sanitizer report, or a case that missed its path)
    got, want = out.stdout.splitlines(), expected_lines()
    assert [l.split()[0] for l in got] == [l.split()[0] for l in want]
    for g, w in zip(got, want):
        assert g == w, "differs in: " + ", ".join(a.split("=")[0] for a, b in zip(g.split(), w.split()) if a != b)
