"""DevProblem::eventFlags (csrc/event_flags.hpp): the launch facts the event phase of the specialised flux kernels of plain launches
tests as bits, made on the host by the pure function event_flags.  No GPU: tests/event_flags_main.cpp -- a host C++17 program over the
header alone -- against the kernels' own expressions (csrc/kernels.hpp, part C of the event phase), restated here in float32:

  kNeedCell        !(uniformSsa >= 0) || uniformSsa < 1 || uniformPf < 1                  the kernels' `needCell` of a one-component domain
  kNoAbsorption    the scattering's albedo is the shared one (uniformSsa >= 0) and `ssa < 1` is false for it
  kWeightStaysOne  never where a weight can change: the cells do not share their albedo, or share one below 1 (w = w * ssa); the
                   surface's reflectance is looked up (a BRDF grid); or a reflection goes on with a factor, `w * albedo > tiny` at w = 1.
                   Set for the benchmark's launch: omega = 1 everywhere over a black surface, and for an albedo of exactly tiny.

Every combination of omega below / at / above 1, shared or per cell (uniformSsa < 0), albedo 0 / tiny / 0.3 / 1, a shared table entry or
none, BRDF grid on / off; and a NaN albedo, a NaN and a negative-zero shared albedo of the cells."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = M.build.CSRC
f32 = np.float32
TINY = np.finfo(np.float32).tiny

OMEGAS = [f32(0.9), f32(1.0) - np.spacing(f32(1.0)) / 2, f32(1.0), f32(1.0) + np.spacing(f32(1.0)), f32(0.0), f32(-0.0), f32(np.nan)]
ALBEDOS = [f32(0.0), f32(TINY), f32(TINY) + np.spacing(f32(TINY)), f32(0.3), f32(1.0), f32(1e-30), f32(-0.1), f32(np.nan)]
COMBINATIONS = [(f32(w) if shared else f32(-1.0), pf, brdf, a)
                for w, shared, pf, brdf, a in itertools.product(OMEGAS, (True, False), (0, 1, 3), (0, 1), ALBEDOS)]


@pytest.fixture(scope="module")
def flags(tmp_path_factory):
    d = tmp_path_factory.mktemp("event_flags")
    exe = d / "event_flags_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "event_flags_main.cpp")])
    rec = np.zeros((len(COMBINATIONS), 4), np.uint32)
    for i, (ssa, pf, brdf, albedo) in enumerate(COMBINATIONS):
        rec[i] = [np.array(ssa, f32).view(np.uint32), np.uint32(pf), np.uint32(brdf), np.array(albedo, f32).view(np.uint32)]
    src, dst = d / "in.bin", d / "out.bin"
    rec.tofile(src)
    subprocess.check_call([str(exe), str(src), str(dst)])
    out = np.fromfile(dst, np.uint32)
    assert out.size == 3 + len(COMBINATIONS)
    return tuple(int(b) for b in out[:3]), out[3:]


def test_three_distinct_bits(flags):
    (stays, none, cell), got = flags
    assert sorted((stays, none, cell)) == [1, 2, 4]
    assert int(np.bitwise_or.reduce(got)) == 7 and all(int(x) & ~7 == 0 for x in got)     # every bit occurs, and no other


def test_flags_are_the_kernels_own_expressions(flags):
    (stays, none, cell), got = flags
    with np.errstate(invalid="ignore"):
        for (ssa, pf, brdf, albedo), f in zip(COMBINATIONS, got):
            what = (float(ssa), pf, brdf, float(albedo), int(f))
            need_cell = (not ssa >= f32(0.0)) or bool(ssa < f32(1.0)) or pf < 1
            shared = bool(ssa >= f32(0.0))                       # the scattering takes uniformSsa (else a per-cell value, any)
            absorbs = (not shared) or bool(ssa < f32(1.0))       # `if (ssa < 1.0f)`
            assert bool(f & cell) == need_cell, what
            assert bool(f & none) == (not absorbs), what
            reflection_goes_on = bool(f32(1.0) * albedo > f32(TINY))     # `w * albedo <= tiny` ends the photon; w = 1 until a weight changes
            can_change = absorbs or brdf != 0 or reflection_goes_on
            if can_change:
                assert not f & stays, what
            if f & stays:
                assert f & none, what                             # (the kernels skip the absorption of such a launch too)


def test_the_benchmark_launch_keeps_its_weights(flags):
    (stays, none, cell), got = flags
    seen = {(float(s), pf, brdf, float(a)): int(f) for (s, pf, brdf, a), f in zip(COMBINATIONS, got) if not np.isnan(s) and not np.isnan(a)}
    assert seen[1.0, 1, 0, 0.0] == stays | none                      # the step cloud: omega = 1, one table entry, black surface
    assert seen[1.0, 1, 0, float(f32(TINY))] == stays | none         # (albedo = tiny: `w * albedo <= tiny` still ends the photon)
    assert seen[1.0, 0, 0, 0.0] == stays | none | cell                # (cells with table entries of their own)
    assert seen[1.0, 1, 0, float(f32(0.3))] == none
    assert seen[1.0, 1, 1, 0.0] == none
    assert seen[float(f32(0.9)), 1, 0, 0.0] == cell
    assert seen[-1.0, 1, 0, 0.0] == cell
