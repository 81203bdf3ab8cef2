"""Wave-uniform and single-lane work taken out of the phases of the specialised flux kernels of plain launches (photon_kernel, STORE;
csrc/kernels.hpp, csrc/tracer.hpp, csrc/event_flags.hpp).

These six kernels -- the field in LDS, read linearly and as column records, each without and with the inverse table in LDS -- wrap a
photon that has crossed a side wall of the periodic domain one axis at a time (x behind the mask of its own compare, y behind its own),
read `needCell`, "nothing absorbs" and "no weight ever leaves 1" as bits of DevProblem::eventFlags, evaluate the roulette block only
where the launch can play and some lane of the event phase does, and make the inverse table's reciprocal length once per wave.  None of
that may show: on every case each kernel gives what the general flux kernel gives on the same launch -- every element of the raw tally
buffer (fluxes, absorption, all eleven counters) with `==` -- and counts what the commit before the change counted
(tests/golden/uniform_event_work_parent.json, tools/record_uniform_event_work.py, which also holds the cases).

The sums are exact, so `==` is the right comparison, by the argument of tests/test_gpu_event_bookkeeping.py: a weight is 1 or a float32
product of factors 0.9 or 0.3 that stays above 2^-16, fewer than 2^13 of them per float64 sum.  The "faint" surface adds weights of
1e-30 (one value: a second reflection ends the photon): a sum that holds a weight of 1 loses every one of them in any order -- 4097
of them are far below half an ulp of 1 --, and a sum of nothing else is a small multiple of one float32 value, exact as well.

  2 x 1 x 2 and 3 x 2 x 4 cells a quarter to three quarters of a free path wide, the sun at mu0 = 0.35 with one azimuth per quadrant,
  4097 photons (one more than a multiple of 64): most steps end on an x or y face and half of those faces -- in y of the first domain
  all of them -- are side walls, crossed in both directions and with cell increments of equal and of opposite sign; each with
    one / one-rr       omega = 1 over a black surface, roulette off and on: the flag path -- no play, three deviates per trace
    absorb / -rr       omega = 0.9, roulette off and on: the absorption region, plays, photons that lose
    lambert            albedo 0.3
    faint              albedo 1e-30 with omega = 1: reflections that end the photon
  step16               the step cloud 32 x 1 x 16, 20001 photons, roulette asked for: the headline's own launch"""
import json

import numpy as np
import pytest

from i3rc_monte_carlo_model_amd import binding as B
from tools import record_uniform_event_work as R

pytestmark = pytest.mark.gpu

IDS = [f"{p}{' table in LDS' if t else ''}" for p, t in R.KERNELS]


@pytest.fixture(scope="module")
def parent():
    return json.load(open(R.GOLDEN))


@pytest.fixture(scope="module")
def general():
    """the general kernel's result of every case at every place of the field: computed once, shared, never written to"""
    out = {}
    for case in R.CASES:
        g = R.integrator(case)
        for place in R.KNOB:
            res = R.run(g, case, place, False, general=True)
            res["raw"].setflags(write=False)
            out[case, place] = res
        g.finalize_Integrator()
    return out


def test_the_cases_cross_the_side_walls(general):
    """what the cases are for: in the small domains a trace is longer than a cell is wide, so it makes more than one voxel step on
    average -- the steps beyond a trace's last one end on a cell face"""
    for case, c in R.CASES.items():
        n = general[case, "GRID_LDS"]["counters"]
        if c["domain"] != "step16":
            assert n["cellSteps"] > n["tracerCalls"], (case, n)


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_equals_general_kernel_and_parent(place, tbl, general, parent):
    assert sorted(parent) == sorted(R.CASES)
    for case, c in R.CASES.items():
        g = R.integrator(case)
        got, ref = R.run(g, case, place, tbl), general[case, place]
        g.finalize_Integrator()
        what = (case, place, tbl)
        assert sorted(got["counters"]) == sorted(B.COUNTER_NAMES), what
        print(what, got["counters"])
        for k in B.COUNTER_NAMES:
            assert got["counters"][k] == ref["counters"][k], (what, k, got["counters"], ref["counters"])
            assert got["counters"][k] == parent[case][k], (what, k, got["counters"], parent[case])
        assert got["raw"].shape == ref["raw"].shape and (got["raw"] == ref["raw"]).all(), (what, np.flatnonzero(got["raw"] != ref["raw"]))
        n = got["counters"]
        assert n["photons"] == c["photons"] and n["scatterings"] > 0, (what, n)
        assert n["tracerCalls"] == n["scatterings"] + n["surfaceHits"] + n["exitsTop"] + n["dropped"], (what, n)
        if c["ssa"] == 1.0 and c["albedo"] == 0.0:
            # the flag path, whether the roulette is asked for or not: no weight leaves 1, nothing is played, and every trace draws its
            # three deviates -- a start or a surviving scattering
            assert n["roulette"] == 0 and n["rngDraws"] == 3 * n["tracerCalls"], (what, n)
            assert n["tracerCalls"] == n["scatterings"] + n["photons"], (what, n)
        if c["ssa"] < 1.0 and c["roulette"]:
            assert 0 < n["roulette"] <= n["scatterings"], (what, n)
            assert n["surfaceHits"] + n["exitsTop"] + n["dropped"] < n["photons"], (what, n)     # (some photons lost their roulette)
        if c["ssa"] < 1.0 and not c["roulette"]:
            assert n["roulette"] == 0, (what, n)
        if c["albedo"] > 0.0:
            assert n["surfaceHits"] > 0 and n["tracerCalls"] > n["scatterings"] + n["photons"], (what, n)   # (reflected photons went on)
        if c["albedo"] == 1e-30:
            # ... and some of them came back to the surface, where the second reflection ended them: fewer photons leave through the
            # top or are dropped than the surface saw arrive for good
            assert n["surfaceHits"] + n["exitsTop"] + n["dropped"] > n["photons"], (what, n)
