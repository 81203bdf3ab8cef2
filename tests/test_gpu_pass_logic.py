"""How the loop of the specialised flux kernels of plain launches (photon_kernel, STORE; csrc/kernels.hpp) decides a pass: stop, run the
event phase, serve the turnover lanes -- the bits of csrc/pass_decision.hpp --, the turnover flag as a 64-bit word joined with the event
phase's masks, the lane states in a numbering of the kernels' own in which `wantTurn` is one compare.  None of that may show: on every case
each of the six kernels -- the field in LDS, in global memory read linearly and as column records, each without and with the inverse table
in LDS -- gives what the general flux kernel gives on the same launch: all eleven counters and every word of the raw tally buffer with `==`.

The cases are chosen for the head's rare arms, not for size:
  photons   1, 3, 4, 5 (the turnover quorum of 4 missed by one, met, passed), 12, 13 (the forcing quorum of 12), 63, 64, 65 (a wavefront
            less one lane, exactly, and one lane alone in a second wave), 4097 (several waves and a launch's end in the middle of one):
            waves with nothing to trace, with one lane alone, and the passes in which a launch runs out of photons;
  domains   1 x 1 x 1 (optical depth 0.3: most events are turnovers), 3 x 5 x 7 (every column its own extinction, optical depth 0.6 ... 2.4)
            and 32 x 1 x 16 (the step cloud's shape, optical depth 2 | 18 in its two halves: many scatterings per photon, the scattering
            quorum decides); every column holds one value over all its layers, which is a field all three places of the field can hold;
  surface   black (a photon that reaches it ends: a turnover lane) and albedo 0.5 (it goes on);
  sun       at the zenith and at mu0 = 0.5, azimuth 40 degrees;
  and, with 4097 photons, the event threshold fixed at the two ends of the adaptive rule's range, 12 and 44.
No absorption in the cells (omega = 1), so a photon's weight is 0.5^k and the float64 sums are exact in any order: `==` is the right
comparison.  Nothing here tries to provoke a fault; `dropped` is compared like every other counter."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from i3rc_monte_carlo_model_amd import binding as B
from tools import record_event_bookkeeping as R

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = (41, 3)
PHOTONS = (1, 3, 4, 5, 12, 13, 63, 64, 65, 4097)
SHAPES = {"1x1x1": (1, 1, 1), "3x5x7": (3, 5, 7), "32x1x16": (32, 1, 16)}
ALBEDOS = (0.0, 0.5)
SUNS = ((1.0, 0.0), (0.5, 40.0))
THRESHOLDS = (12, 44)      # fixed event thresholds, run with the largest photon count; 0 = the adaptive rule
IDS = [f"{p}{' table in LDS' if t else ''}" for p, t in R.KERNELS]


def launches():
    """(photons, sun, event threshold) of every launch on one domain with one surface"""
    return [(n, sun, 0) for n in PHOTONS for sun in SUNS] + [(PHOTONS[-1], SUNS[1], thr) for thr in THRESHOLDS]


def domain(which):
    nx, ny, nz = SHAPES[which]
    n = nx * ny
    if which == "1x1x1":
        tau = np.full(n, f32(0.3))
    elif which == "3x5x7":
        tau = f32(0.6) + f32(1.8) * np.arange(n, dtype=f32) / f32(n - 1)
    else:
        tau = np.where(np.arange(n) < n // 2, f32(2.0), f32(18.0)).astype(f32)
    ze = (np.arange(nz + 1, dtype=f32) / f32(nz)).astype(f32)                  # layers of equal depth, 1 in all
    ext = np.broadcast_to(tau.reshape(1, ny, nx), (nz, ny, nx)).astype(f32)   # (extinction = optical depth: the domain is 1 deep)
    return dict(xe=(f32(0.25) * np.arange(nx + 1)).astype(f32), ye=(f32(0.25) * np.arange(ny + 1)).astype(f32), ze=ze, ext=ext,
                ssa=np.ones(ext.shape, f32), pf=np.ones(ext.shape, np.int32))


def integrator(which, albedo, place):
    d = domain(which)
    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    dom.addOpticalComponent("cloud", d["ext"], d["ssa"], d["pf"], M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]))
    g = M.new_Integrator(dom)
    g.specifyParameters(surfaceAlbedo=albedo, useRussianRoulette=False)
    g.select_grid_place(R.KNOB[place])
    return g


def run(g, kernel, photons, sun, threshold):
    g.set_tuning(evThreshold=threshold, kernel=kernel)
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*sun, photons), firstPhoton=0)
    res = g.finish()
    return res, g.kernel_name()


@pytest.fixture(scope="module")
def general():
    """per domain, surface and place of the field: the integrator (shared with the tests, which only launch on it) and the general kernel's
    result of every launch: computed once, never written to"""
    out = {}
    for place in ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS"):
        for which in SHAPES:
            for albedo in ALBEDOS:
                g = integrator(which, albedo, place)
                ref = {}
                for photons, sun, thr in launches():
                    res, name = run(g, "general", photons, sun, thr)
                    assert name == R.kernel_name(place, False, True), name
                    res["raw"].setflags(write=False)
                    ref[photons, sun, thr] = res
                out[which, albedo, place] = (g, ref)
    yield out
    for g, _ in out.values():
        g.finalize_Integrator()


def test_the_cases_reach_the_rare_arms(general):
    """every photon is accounted for, photons end at both boundaries where there are enough of them, and a reflecting surface sends them on"""
    for (which, albedo, place), (_, ref) in general.items():
        for (photons, sun, thr), res in ref.items():
            n = res["counters"]
            what = (which, albedo, place, photons, sun, thr)
            assert n["photons"] == photons, (what, n)
            assert n["tracerCalls"] == n["scatterings"] + n["surfaceHits"] + n["exitsTop"] + n["dropped"], (what, n)
            if photons >= 63:
                assert n["scatterings"] > 0 and n["surfaceHits"] + n["exitsTop"] > 0, (what, n)
            if photons == PHOTONS[-1]:      # (enough photons for both boundaries, whatever the optical depth)
                assert n["exitsTop"] > 0 and n["surfaceHits"] > 0, (what, n)
            if albedo == 0.0:
                assert n["surfaceHits"] + n["exitsTop"] + n["dropped"] == photons, (what, n)


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_equals_general_kernel(place, tbl, general):
    for which in SHAPES:
        for albedo in ALBEDOS:
            g, ref = general[which, albedo, place]
            for photons, sun, thr in launches():
                got, name = run(g, "auto" if tbl else "lane", photons, sun, thr)
                want = ref[photons, sun, thr]
                what = (which, albedo, place, tbl, photons, sun, thr)
                assert name == R.kernel_name(place, tbl), (what, name)
                assert sorted(got["counters"]) == sorted(B.COUNTER_NAMES), what
                for k in B.COUNTER_NAMES:
                    assert got["counters"][k] == want["counters"][k], (what, k, got["counters"], want["counters"])
                assert got["raw"].shape == want["raw"].shape and (got["raw"] == want["raw"]).all(), (what, np.flatnonzero(got["raw"] != want["raw"]))
