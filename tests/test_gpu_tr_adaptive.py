"""Variable-step transient on the MI355X (pe_hip_analyze_tr_adaptive, include/pe_hip.h): the properties of tests/test_tr_adaptive_emu.py
on the real library -- k_tr_lte, k_tr_history_push and k_tr_state_copy behind the controller -- plus the Monte-Carlo sweep's size.
Every case is a child process of its own under a time limit; once a child has died of a signal or run out of time nothing more is started
on the GPU (the remaining cases fail without running)."""
import subprocess
import sys

import pytest

from test_tr_adaptive_emu import ACCURACY, BATCH, IDS, NAN_STATE, PINNED, PRE, REPLAY_BRIDGE, RESCUE, RULES, SCHEDULES, SOURCE_BP

_gpu_lost = []


def run_gpu(body, timeout=600):
    if _gpu_lost:
        pytest.fail(f"not started: an earlier GPU case ended abnormally ({_gpu_lost[0]})")
    try:
        r = subprocess.run([sys.executable, "-c", PRE + body], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _gpu_lost.append("time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append(f"exit status {r.returncode}")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_pinned_controller_equals_fixed_step_bitwise(knobs):
    assert "ok" in run_gpu(PINNED % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_replay_with_fixed_step_calls_reproduces_every_accepted_point(knobs):
    assert "ok" in run_gpu(REPLAY_BRIDGE % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_has_one_sequence_decided_by_the_worst_instance(knobs):
    assert "ok" in run_gpu(BATCH % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_accuracy_and_economy_against_analytic_and_reference_runs(knobs):
    out = run_gpu(ACCURACY % knobs)
    print(out)
    assert "ok" in out


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_step_cutting_rescues_a_failing_run(knobs):
    assert "ok" in run_gpu(RESCUE % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_window_rules_and_refused_arguments(knobs):
    assert "ok" in run_gpu(RULES % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_source_breakpoints_of_every_generator_kind(knobs):
    assert "ok" in run_gpu(SOURCE_BP % knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_a_nan_in_the_state_is_never_accepted(knobs):
    """k_tr_lte's wavefront reduction, ballot and atomics see a NaN candidate in one instance of five"""
    assert "ok" in run_gpu(NAN_STATE % knobs)


# the Monte-Carlo sweep's size: 1 024 instances of the non-linear 100 x 100 mesh (10 002 rows), the default schedule of that batch
SWEEP = r'''
B, W, N = 1024, 100, 20
deck, r, c = D.rc_mesh_params(W, W, list(range(1, B + 1)), True)
ov = {"R": r[:, :, None], "C": c[:, :, None]}
nn = deck.n_nodes
ROWS = [0, 1, W + 1, nn // 2, nn - 2, nn - 1, nn, W * W - 1]      # mesh nodes, the source node, the source's branch current
# pinned controller against the fixed step, bit for bit
res = []
for adaptive in (False, True):
    e = engine(deck, B, ov)
    e.set_probes(ROWS, N + 1, 1, [("max", 0), ("integ", 6)])
    e.arm_probes()
    if adaptive:
        st = e.analyze_tr_adaptive(1.0, 1e-10, dt_min=1e-10, dt_max=1e-10, lte_reltol=-1.0, max_steps=N)
        assert st["n_accepted"] == N and st["run"]["steps"] == B * N, st
    else:
        e.analyze_tr(1e-10, N)
    s = e.state()
    res.append((e.solution(), s["t"], s["steps"], s["iters"], s["status"], e.newton_trace(), *e.probe_samples(), e.measures()))
    e.close()
for k, (a, b) in enumerate(zip(*res)):
    assert np.array_equal(a, b, equal_nan=True), k
del res
# free-running for N attempted steps: the recorded decisions are consistent with q recomputed from the probed rows (a lower bound of
# the q over all rows that decided)
e = engine(deck, B, ov)
e.set_probes(ROWS, N + 1, 1)
e.arm_probes()
tol = dict(lte_reltol=1e-3, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0)
st = e.analyze_tr_adaptive(1e-7, 2e-11, max_steps=N, **tol)
dt, oc = e.tr_step_log()
assert st["rc"] == 0 and len(dt) == N and st["n_accepted"] + st["n_rejected_lte"] + st["n_rejected_newton"] == N and st["t_end"] < 1e-7, st
t, x = samples(e)
assert len(t) == st["n_accepted"] + 1 and np.all(np.diff(t) > 0) and t[-1] == st["t_end"] == e.state()["t"][0]
node = np.array([rw < nn for rw in ROWS])
def q_rows(a):
    tt, xx, h = t[a - 2:a + 2], x[a - 2:a + 2], t[a + 1] - t[a]
    d10, d21, dn2 = (xx[1] - xx[0]) / (tt[1] - tt[0]), (xx[2] - xx[1]) / (tt[2] - tt[1]), (xx[3] - xx[2]) / (tt[3] - tt[2])
    dd3 = ((dn2 - d21) / (tt[3] - tt[1]) - (d21 - d10) / (tt[2] - tt[0])) / (tt[3] - tt[0])
    tl = 7.0 * (1e-3 * np.maximum(np.abs(xx[3]), np.abs(xx[2])) + np.where(node, 1e-6, 1e-9))
    return float(np.max(0.5 * h * h * h * np.abs(dd3) / tl))
acc = np.flatnonzero(oc == 0)
tested = 0
for a, k in enumerate(acc):
    assert t[a + 1] == t[a] + dt[k]
    if a >= 3:                                   # the first three steps of an empty history are untested
        q8 = q_rows(a)
        assert q8 <= 1 + 1e-9, (a, q8)
        tested += 1
        if k + 1 < N:
            grow = min(2.0, 0.9 * q8 ** (-1.0 / 3.0)) if q8 > 0 else 2.0
            assert dt[k + 1] <= dt[k] * grow * (1 + 1e-9), (k, dt[k + 1], dt[k], grow)   # the deciding q is at least q8
    elif k + 1 < N:
        assert dt[k + 1] == dt[k], "no growth before the history is full"
assert tested >= 5, (tested, oc)
print("ok", st["n_accepted"], st["n_rejected_lte"], st["n_rejected_newton"], st["run"]["gpu_ms"])
'''


@pytest.mark.gpu
def test_sweep_size_runs_and_stays_bit_identical_when_pinned():
    out = run_gpu(SWEEP, timeout=900)
    print(out)
    assert "ok" in out
