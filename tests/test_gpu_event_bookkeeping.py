"""The event phase's bookkeeping in the specialised flux kernels of plain launches (photon_kernel, STORE; csrc/kernels.hpp).

These six kernels -- the field in LDS, read linearly and as column records, each without and with the inverse table in LDS -- do not
count tracer calls (they are the launch's scatterings + surface arrivals + exits through the top + dropped photons), count roulette
plays only in a launch that plays roulette, take the counts of endings and scatterings from the masks of the two height compares, and
skip the endings and the hand-out of new photons in an event phase that serves neither.  None of that may show: on every case each
kernel gives what the general flux kernel gives on the same launch -- every element of the raw tally buffer (fluxes, absorption, all
eleven counters) with `==` -- and counts what the commit before the change counted (tests/golden/event_bookkeeping_parent.json,
tools/record_event_bookkeeping.py, which also holds the cases).

The sums are exact, so `==` is the right comparison: a weight is 1, or a float32 product of factors 0.9 or 0.3 that stays above 2^-16
in these thin clouds (some hundred scatterings would be needed); the 4097 photons of such a case put fewer than 2^13 weights into one
float64 sum, and 13 + 16 + 24 bits fit a float64's 53 whatever the order.  (An absorbed part is a tenth of a weight, and the 2^15
scatterings of a launch spread over the cells: the same count of bits.)

  a  3 x 2 x 4 cells, 4097 photons (one more than a multiple of 64)           more than one fill of a wave's start store
  b  the step cloud 32 x 1 x 16, 20001 photons                                 the headline's own shape
  c  (a) over a surface of albedo 0.3                                          reflections go on: the derived tracer calls
  d  (a) with omega = 0.9, Russian roulette on and off                         the roulette counter and the roulette ending
  e  (a) with the sun at mu0 = 0.35                                            endings at the top and at the surface in one event phase"""
import json

import numpy as np
import pytest

from i3rc_monte_carlo_model_amd import binding as B
from tools import record_event_bookkeeping as R

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


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_equals_general_kernel_and_parent(place, tbl, general, parent):
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
        if c["albedo"] == 0.0 and not c["roulette"]:
            # a black surface, no roulette: a trace starts at a photon's start and after every scattering, nowhere else
            assert n["tracerCalls"] == n["scatterings"] + n["photons"], (what, n)
            assert n["roulette"] == 0 and n["surfaceHits"] + n["exitsTop"] + n["dropped"] == n["photons"], (what, n)
        if c["roulette"]:
            assert 0 < n["roulette"] <= n["scatterings"], (what, n)
            assert n["surfaceHits"] + n["exitsTop"] + n["dropped"] < n["photons"], (what, n)     # (some photons lost their roulette)
        if c["albedo"] > 0.0:
            assert n["tracerCalls"] > n["scatterings"] + n["photons"], (what, n)                 # (reflected photons went on)
        if case == "e":
            assert n["exitsTop"] > 0 and n["surfaceHits"] > 0, (what, n)
