"""CPU: tests/cpp/engine_lifecycle.cpp as ONE stand-alone program under AddressSanitizer + UBSan + LeakSanitizer.  The engine's
translation units and the host emulation of the kernels are compiled into the executable against the HIP shim of tests/emu (no shared
library, nothing preloaded), so every allocation of the engine object is instrumented: an engine, event, pinned buffer or sub-engine
that is not released when its owner goes is a leak report, one released twice a crash.  The shim's events are heap objects (a missing
hipEventDestroy shows); its stream is a null handle, so the stream's ownership is checked by reading.  The build also switches on the
unit checks of the owning types of pe_engine_internal.hpp (Pinned, Event, Stream, EnginePtr; a fresh DcSweep / Ac::Sweep / Ac
assigned over a built one).  The error paths of the graph capture in pe_kernels.hip need a failing launch and are checked by reading."""
import os
import subprocess

from parity_common import ROOT, make

CPP = os.path.join(ROOT, "tests", "cpp")


def test_engine_lifecycle_is_clean_under_sanitizers():
    make("-j8", "-C", CPP, "asan")
    out = subprocess.run([os.path.join(CPP, "_build_asan", "engine_lifecycle")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"engine_lifecycle (sanitized) exited {out.returncode}: {out.stderr}"
    assert out.stderr == "", out.stderr
