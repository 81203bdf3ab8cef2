"""What a wave of the specialised flux kernels of plain launches does in one pass of its loop (csrc/pass_decision.hpp): stop, run the
event phase, serve the turnover lanes -- one small integer made by 32-bit arithmetic from the head's lane counts.  No GPU:
tests/pass_decision_main.cpp -- a host C++17 program over the header alone, which the kernels include too -- against the three boolean
expressions the loop spelt before, written out here:

  stop     = nSc == 0 and nTu == 0 and trEmpty
  runEvent = nSc + nTu > 0 and (nSc >= evThr or nTu >= kTurnForce or trEmpty)
  doTurn   = nTu >= kTurnMin or trEmpty or nSc == 0

for every nSc, nTu >= 0 with nSc + nTu <= 64 (a wavefront), both values of trEmpty, every event threshold a launch can have (1 ... 64:
the fixed ones of set_tuning; the adaptive rule stays within 12 ... 44) and the quorums 4 / 12 (tuning.hpp) and 1 / 1.

A wrong decision is an endless loop on the GPU, so two properties are asserted on their own as well: with all three masks empty the
wave stops, and a wave that does not stop makes progress -- it runs an event phase or has a lane to trace."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = M.build.CSRC
STOP, EVENT, TURN = 1, 2, 4
QUORUMS = [(4, 12), (1, 1)]
THRESHOLDS = range(1, 65)


def records():
    counts = [(a, b) for a in range(65) for b in range(65 - a)]
    out = [(a, b, e, thr, q) for q in range(len(QUORUMS)) for thr in THRESHOLDS for e in (0, 1) for a, b in counts]
    return np.array(out, np.int32)


@pytest.fixture(scope="module")
def decided(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_decision")
    exe = d / "pass_decision_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "pass_decision_main.cpp")])
    recs = records()
    src, dst = d / "in.bin", d / "out.bin"
    recs.tofile(src)
    subprocess.check_call([str(exe), str(src), str(dst)])
    out = np.fromfile(dst, np.int32)
    assert out.size == len(recs)
    return recs, out


def test_the_cases_cover_what_the_kernels_meet():
    recs = records()
    assert len(recs) == 65 * 66 // 2 * 2 * len(THRESHOLDS) * len(QUORUMS)
    assert set(range(12, 45)) <= set(recs[:, 3].tolist())
    assert (recs[:, 0] + recs[:, 1]).max() == 64 and recs[:, :2].min() == 0
    for name, value in (("I3RC_STORE_TURN_MIN", 4), ("I3RC_STORE_TURN_FORCE", 12)):   # (the first pair of quorums is the kernels')
        text = open(os.path.join(CSRC, "tuning.hpp")).read()
        assert f"#define {name} {value}\n" in text, name


def test_decision_equals_the_three_expressions(decided):
    recs, out = decided
    nSc, nTu, thr = recs[:, 0], recs[:, 1], recs[:, 3]
    empty = recs[:, 2] != 0
    kMin = np.array([q[0] for q in QUORUMS])[recs[:, 4]]
    kForce = np.array([q[1] for q in QUORUMS])[recs[:, 4]]
    stop = (nSc == 0) & (nTu == 0) & empty
    run = (nSc + nTu > 0) & ((nSc >= thr) | (nTu >= kForce) | empty)
    turn = (nTu >= kMin) | empty | (nSc == 0)
    # (where the wave stops the loop tests STOP first and leaves: the function sets the other two bits there -- the turnover lanes' one as the
    # expression has it, the event's although the expression says no, which saves clearing it at every pass -- and nobody reads them)
    assert not (run & stop).any() and turn[stop].all()
    want = stop * STOP + (run | stop) * EVENT + turn * TURN
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (recs[bad[:5]], out[bad[:5]], want[bad[:5]])
    assert stop.any() and run.any() and (~run & ~stop).any() and (~turn).any()


def test_a_wave_with_nothing_left_stops(decided):
    recs, out = decided
    nothing = (recs[:, 0] == 0) & (recs[:, 1] == 0) & (recs[:, 2] != 0)
    assert nothing.sum() == len(THRESHOLDS) * len(QUORUMS)
    assert ((out[nothing] & STOP) != 0).all()
    assert ((out[~nothing] & STOP) == 0).all()      # ... and no other wave does


def test_a_wave_that_goes_on_makes_progress(decided):
    recs, out = decided
    goes_on = (out & STOP) == 0
    assert goes_on.any()
    traces = recs[:, 2] == 0
    assert (((out & EVENT) != 0) | traces)[goes_on].all()
    # an event phase has somebody to serve: a lane with an interaction due, or turnover lanes that it takes
    served = (recs[:, 0] > 0) | ((recs[:, 1] > 0) & ((out & TURN) != 0))
    assert served[goes_on & ((out & EVENT) != 0)].all()
