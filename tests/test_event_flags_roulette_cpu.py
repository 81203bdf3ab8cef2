"""The roulette bit of DevProblem::eventFlags (csrc/event_flags.hpp, kPlaysRoulette): "this launch can play Russian roulette", which the
event phase of the specialised flux kernels of plain launches tests as one bit where it used to ask two things.  No GPU:
tests/event_flags_roulette_main.cpp -- a host C++17 program over the header alone -- against the kernels' own expression (csrc/kernels.hpp,
part C of the event phase, and the roulette count behind it), restated here:

  kPlaysRoulette   Pe.useRR && (Pe.eventFlags & kWeightStaysOne) == 0u

and the word that event_flags made before the bit existed, restated here in float32 too: the call with four arguments -- the callers from
before -- returns exactly that word, and the fifth argument changes nothing but the new bit.

The grid: the cells' shared albedo NaN, -0, +0, the smallest normal float, 0.9, the floats next to 1 on both sides, 1, and per-cell values
(uniformSsa < 0); a shared table entry or none; BRDF grid on / off; the surface's albedo NaN, -0, +0, the smallest normal float, the float
above it, 1e-30, 0.3, 1; roulette off / on.  The program is built and run a second time with the address and undefined-behaviour
sanitizers, as a program of its own."""
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
TINY = np.finfo(np.float32).tiny    # FLT_MIN

ONE = f32(1.0)
OMEGAS = [f32(np.nan), f32(-0.0), f32(0.0), f32(TINY), f32(0.9), ONE - np.spacing(ONE) / 2, ONE, ONE + np.spacing(ONE), f32(-1.0)]
ALBEDOS = [f32(np.nan), f32(-0.0), f32(0.0), f32(TINY), f32(TINY) + np.spacing(f32(TINY)), f32(1e-30), f32(0.3), ONE]
GRID = list(itertools.product(OMEGAS, (0, 1, 3), (0, 1), ALBEDOS, (0, 1)))   # uniformSsa, uniformPf, brdfGrid, albedo, useRoulette


def run_program(d, extra):
    exe = d / "event_flags_roulette_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", *extra, "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "event_flags_roulette_main.cpp")])
    rec = np.zeros((len(GRID), 5), np.uint32)
    for i, (ssa, pf, brdf, albedo, roulette) in enumerate(GRID):
        rec[i] = [np.array(ssa, f32).view(np.uint32), np.uint32(pf), np.uint32(brdf), np.array(albedo, f32).view(np.uint32), np.uint32(roulette)]
    src, dst = d / "in.bin", d / "out.bin"
    rec.tofile(src)
    subprocess.check_call([str(exe), str(src), str(dst)])
    out = np.fromfile(dst, np.uint32)
    assert out.size == 4 + 2 * len(GRID)
    return tuple(int(b) for b in out[:4]), out[4:].reshape(len(GRID), 2)


@pytest.fixture(scope="module")
def flags(tmp_path_factory):
    return run_program(tmp_path_factory.mktemp("event_flags_roulette"), [])


def word_before(ssa, pf, brdf, albedo):
    """event_flags as it was before the roulette bit, in float32 (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        f = 0
        none = bool(ssa >= ONE)
        if none:
            f |= 2
        if none and not brdf and bool(albedo <= f32(TINY)):
            f |= 1
        if (not bool(ssa >= f32(0.0))) or bool(ssa < ONE) or pf < 1:
            f |= 4
        return f


def test_four_distinct_bits(flags):
    bits, got = flags
    assert bits[:3] == (1, 2, 4)                      # (the three from before keep their values)
    assert bits[3] == 8
    assert int(np.bitwise_or.reduce(got[:, 1])) == 15 and not (got & ~np.uint32(15)).any()


def test_the_four_argument_call_returns_what_it_returned(flags):
    _, got = flags
    for (ssa, pf, brdf, albedo, roulette), (four, _) in zip(GRID, got):
        assert int(four) == word_before(ssa, pf, brdf, albedo), (float(ssa), pf, brdf, float(albedo), int(four))


def test_the_roulette_bit_is_the_kernels_own_expression(flags):
    (stays, none, cell, plays), got = flags
    seen = set()
    for (ssa, pf, brdf, albedo, roulette), (four, five) in zip(GRID, got):
        what = (float(ssa), pf, brdf, float(albedo), roulette, int(four), int(five))
        four, five = int(four), int(five)
        assert five & ~plays == four, what                       # the fifth argument changes no other bit
        use_rr = roulette != 0                                    # DevProblem::useRR
        assert bool(five & plays) == (use_rr and (four & stays) == 0), what
        seen.add((bool(five & stays), bool(five & plays)))
    assert seen == {(False, False), (False, True), (True, False)}   # (weights that stay 1 and a roulette: never both)


def test_the_benchmark_launch_plays_no_roulette(flags):
    (stays, none, cell, plays), got = flags
    seen = {(float(s), pf, brdf, float(a), r): int(five) for (s, pf, brdf, a, r), (_, five) in zip(GRID, got)
            if not np.isnan(s) and not np.isnan(a) and not np.signbit(a) and not np.signbit(s)}
    assert seen[1.0, 1, 0, 0.0, 1] == stays | none                   # the step cloud: omega = 1 over a black surface, roulette asked for
    assert seen[1.0, 1, 0, float(f32(0.3)), 1] == none | plays       # a reflection that goes on halves the weight: the roulette can play
    assert seen[1.0, 1, 0, float(f32(0.3)), 0] == none
    assert seen[float(f32(0.9)), 1, 0, 0.0, 1] == cell | plays
    assert seen[1.0, 1, 1, 0.0, 1] == none | plays                   # (a BRDF grid: the reflectance is looked up)


def test_the_program_under_the_sanitizers_says_the_same(flags, tmp_path):
    bits, got = run_program(tmp_path, ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
    assert bits == flags[0] and (got == flags[1]).all()
