"""The first flight of a zenith sun's photons from a column table (csrc/first_flight.hpp; photon_kernel, FLIGHT): the specialised flux
kernels of plain launches look a photon's first optical depth up in its start column's cumulative optical path where they make its start,
and hand the photon out where its first scattering happens -- or below the grid.  None of that may show: each of the six kernels -- the
field in LDS, in global memory read linearly and as column records, each without and with the inverse table in LDS -- is run with the
table ON and with it OFF (set_tuning(firstFlightTable=...)) against the general flux kernel on the same launch: all eleven counters and
every word of the raw tally buffer with `==`, by the rules of tests/test_gpu_scalar_relief.py for launches whose weights only halve
(the rules' helpers live in tools/record_event_bookkeeping.py).  `cellSteps` in particular: the landed steps are counted by the fill, not executed.

  domains   1 x 1 x 1, optical depth 0.3: most photons go through the bottom;
            3 x 5 x 7, every column its own extinction, present only in layers 3 ... 5: clear air above and below the cloud, a run that
            column records can hold;  the same with one column entirely clear;
            32 x 1 x 16, optical depth 2 | 18 in its two halves: the step cloud's shape;
  photons   1, 63, 64, 65, 4097;  firstPhoton 0 and 2^32 - 40 (the carry into the high counter word of the fill's Philox block);
  sun       at the zenith with azimuth 0 and 200 degrees (solarDy = -0), and mu0 = 0.5, where the launch must not land;
  surface albedo 0 and 0.5 (a photon through the bottom ends, or reflects), single-scattering albedo 1 and 0.5 (the landed scattering
            absorbs in the cell of the packed index), roulette off and on.
The reference's reruns.  Where weights only halve (omega = 0.5 without the roulette) a float64 sum of addends 2^-j can depend on the order
in which they arrive, and test_gpu_scalar_relief.py's two rules decide each such launch: provably exact, or the spread of the general
kernel's own RERUNS runs -- `==` where they agree word for word, four times their spread where they do not.  There the reruns repeat the
launch as it is, which shows an order dependence only where the order itself varies from run to run: several workgroups.  A launch of
one or two waves (1 ... 65 photons) adds in the same order every time, and every kernel of the parent kept that order, because all of
them visit their event phases by the same rule.  A landed photon scatters in the phase in which it is handed out, one event phase
earlier than it used to: the ORDER of a wave's additions is what this change changes, by design.  So the reruns here vary what only
schedules -- the event threshold (set_tuning: 1 and 64 beside the adaptive default; no photon path depends on it) -- and the spread
is the reference's own under another order of the same additions.  The rules, RERUNS and the factor four are that file's, and so are
its two guards on the spread, asserted where every reference is made (reference()): a provably exact launch and a launch of one photon
rerun equal, and no spread exceeds 16 * 2^-52 -- the tolerance is at most 64 * 2^-52 of a word, never open-ended.  The counters stay
`==` on every launch.  (First seen on the GPU: 32 x 1 x 16, omega 0.5, 63 photons from 2^32 - 40 on, all eleven counters equal,
two tally words -- fluxDown of column 11, the absorption of cell (8, 1, 1) -- unequal to the general kernel's single order.)

Two more domains cover the edges of eligibility: the 3 x 5 x 7 domain with its x and y edges starting at 4096 (cell width 0.25), where
photons within two spacings of their forward edge -- which are not landed -- are common: they are counted on the CPU first, from Philox
alone; and the same domain with z0 = 4096, whose start height rounds to zMax: not eligible.
Nothing here tries to provoke a fault."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from i3rc_monte_carlo_model_amd import binding as B
from tests import stream_model as S
from tools import record_event_bookkeeping as R

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = (43, 7)
PHOTONS = (1, 63, 64, 65, 4097)
FIRSTS = (0, 2 ** 32 - 40)
SUNS = ((1.0, 0.0), (1.0, 200.0), (0.5, 40.0))
ALBEDOS = (0.0, 0.5)
SSAS = (1.0, 0.5)
ROULETTES = (False, True)
DOMAINS = ("1x1x1", "3x5x7", "3x5x7 clear column", "32x1x16")
PLACES = ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS")
IDS = [f"{p}{' table in LDS' if t else ''}" for p, t in R.KERNELS]
EDGE_LAUNCH = (0.0, False, 4097, (1.0, 0.0), 0)         # the launch of the two domains at the edges of eligibility
MIN_NEAR_EDGE = 8


def field(which, origin=0.0, z0=0.0):
    """x, y and z edges and the extinction [nz][ny][nx] of a domain"""
    nx, ny, nz = {"1": (1, 1, 1), "3": (3, 5, 7)}.get(which[0], (32, 1, 16))
    xe = (f32(origin) + f32(0.25) * np.arange(nx + 1, dtype=f32)).astype(f32)
    ye = (f32(origin) + f32(0.25) * np.arange(ny + 1, dtype=f32)).astype(f32)
    if z0 != 0.0:
        ze = (f32(z0) + f32(0.125) * np.arange(nz + 1, dtype=f32)).astype(f32)     # (a depth of 0.875: the start height rounds to zMax)
    else:
        ze = (np.arange(nz + 1, dtype=f32) / f32(nz)).astype(f32)
    ext = np.zeros((nz, ny, nx), f32)
    if which == "1x1x1":
        ext[:] = f32(0.3)
    elif which.startswith("3x5x7"):
        tau = f32(0.6) + f32(1.8) * np.arange(nx * ny, dtype=f32).reshape(ny, nx) / f32(nx * ny - 1)
        ext[2:5] = (tau / (ze[5] - ze[2]))[None]                                    # layers 3 ... 5 (1-based)
        if which.endswith("clear column"):
            ext[:, 2, 1] = f32(0.0)
    else:
        ext[:] = np.where(np.arange(nx) < nx // 2, f32(2.0), f32(18.0)).astype(f32)[None, None, :]
    return xe, ye, ze, ext


def settings():
    return [(which, ssa) for which in DOMAINS for ssa in SSAS]


def launches():
    """(surface albedo, roulette, photons, sun, firstPhoton) of every launch on one integrator"""
    return [(a, rr, n, sun, first) for a in ALBEDOS for rr in ROULETTES for n in PHOTONS for sun in SUNS for first in FIRSTS]


def integrator(which, ssa, place, **where):
    xe, ye, ze, ext = field(which, **where)
    dom = M.new_Domain(xe, ye, ze)
    dom.addOpticalComponent("cloud", ext, np.full(ext.shape, f32(ssa)), np.ones(ext.shape, np.int32), M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]))
    g = M.new_Integrator(dom)
    g.select_grid_place(R.KNOB[place])
    return g


def run(g, kernel, launch, table=None, threshold=0):
    albedo, roulette, photons, sun, first = launch
    g.specifyParameters(surfaceAlbedo=albedo, useRussianRoulette=roulette)
    g.set_tuning(evThreshold=threshold, kernel=kernel, firstFlightTable=table)
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*sun, photons), firstPhoton=first)
    res = g.finish()
    return res, g.kernel_name(), g.first_flight_landed()


RERUN_THRESHOLDS = (1, 64)                              # event thresholds of the general kernel's reruns (0, the adaptive default, is the first run's)


def reference(g, place, setting, todo):
    """the general kernel's result of every launch and, where weights only halve, the spread of its own reruns (test_gpu_scalar_relief.py)
    -- each rerun at another event threshold: see the module's text"""
    ref, spread = {}, {}
    assert len(RERUN_THRESHOLDS) == R.RERUNS - 1
    for launch in todo:
        res, name, landed = run(g, "general", launch)
        assert name == R.kernel_name(place, False, True) and not landed, (name, landed)
        res["raw"].setflags(write=False)
        ref[launch] = res
        if R.weights_only_halve(setting, launch):
            again = [run(g, "general", launch, threshold=t)[0] for t in RERUN_THRESHOLDS]
            assert all(a["counters"] == res["counters"] for a in again), (place, setting, launch)
            spread[launch] = R.spread_of([res["raw"]] + [a["raw"] for a in again])
            # that file's two guards on the spread, under the varied thresholds too: a provably exact launch and a launch of one photon
            # (its addends arrive in its own order) rerun equal, and no spread exceeds a few units of the last place -- so that
            # four times the spread is never more than 64 * 2^-52 of a word
            what = (place, setting, launch, spread[launch])
            if R.provably_exact(launch, res["counters"]) or launch[2] == 1:
                assert spread[launch] == 0.0, what
            assert spread[launch] <= R.MAX_SPREAD, what
    return ref, spread


@pytest.fixture(scope="module")
def general():
    """per place of the field and setting: the integrator (shared with the tests, which only launch on it) and the general kernel's
    results: computed once, never written to"""
    out = {}
    for place in PLACES:
        for setting in settings():
            g = integrator(*setting, place)
            out[place, setting] = (g,) + reference(g, place, setting, launches())
    yield out
    for g, _, _ in out.values():
        g.finalize_Integrator()


def same(got, want, spread, what):
    assert sorted(got["counters"]) == sorted(B.COUNTER_NAMES), what
    for k in B.COUNTER_NAMES:
        assert got["counters"][k] == want["counters"][k], (what, k, got["counters"], want["counters"])
    assert got["raw"].shape == want["raw"].shape, what
    if spread > 0.0 and not R.provably_exact(what[-1], want["counters"]):     # (the reference's own reruns differ)
        off = np.abs(got["raw"] - want["raw"]) > 4.0 * spread * np.abs(want["raw"])
        assert not off.any(), (what, spread, np.flatnonzero(off))
    else:
        assert (got["raw"] == want["raw"]).all(), (what, np.flatnonzero(got["raw"] != want["raw"]))


def check(g, ref, spread, place, tbl, setting, todo, eligible):
    for launch in todo:
        steps = {}
        for table in (True, False):
            got, name, landed = run(g, "auto" if tbl else "lane", launch, table)
            what = (place, tbl, setting, table, launch)
            assert name == R.kernel_name(place, tbl), (what, name)          # the kernel's name is what it was
            assert landed == (table and eligible(launch)), (what, landed)
            same(got, ref[launch], spread.get(launch, 0.0), what)
            steps[table] = got["counters"]["cellSteps"]
        assert steps[True] == steps[False], (place, tbl, setting, launch, steps)
    g.set_tuning(firstFlightTable=True)


def test_the_cases_reach_the_arms(general):
    """photons go through the bottom and end or reflect there, land and scatter, absorb and play roulette; the identity of the tracer
    calls holds"""
    for (place, setting), (_, ref, _) in general.items():
        which, ssa = setting
        for launch, res in ref.items():
            albedo, roulette, photons, sun, first = launch
            n = res["counters"]
            what = (place, setting, launch, n)
            assert n["photons"] == photons, what
            assert n["tracerCalls"] == n["scatterings"] + n["surfaceHits"] + n["exitsTop"] + n["dropped"], what
            if photons == PHOTONS[-1]:
                assert n["scatterings"] > 0 and n["surfaceHits"] > 0, what
                if which == "1x1x1" and sun[0] == 1.0:
                    assert n["surfaceHits"] > photons // 2, what                   # most photons go through the bottom
                if roulette and ssa == 0.5 and which != "1x1x1":
                    assert n["roulette"] > 0, what


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_with_and_without_the_table_equals_general_kernel(place, tbl, general):
    for setting in settings():
        g, ref, spread = general[place, setting]
        check(g, ref, spread, place, tbl, setting, launches(), lambda launch: launch[3][0] == 1.0)


def near_edge_photons(origin):
    """photons 0 ... 4096 of SEED on the 3 x 5 x 7 domain whose start lies within two spacings of its forward x or y edge: the start as
    the kernels make it (part B of the event phase), from Philox alone"""
    xe, ye, _, _ = field("3x5x7", origin=origin)
    n = EDGE_LAUNCH[2]
    block = S.philox(np.arange(n, dtype=np.uint64), np.zeros(n, np.uint64), 0, 0, SEED[0], SEED[1])
    near = np.zeros(n, bool)
    for word, e in ((block[0], xe), (block[1], ye)):
        cells = len(e) - 1
        x = (e[0] + S.unit(word).astype(f32) * f32(e[-1] - e[0])).astype(f32)
        c = np.minimum(((x - e[0]).astype(f32) / f32(e[1] - e[0])).astype(f32).astype(np.int64) + 1, cells)
        c = c + (np.abs(e[c] - x) < np.spacing(x))
        c = np.where(c == cells + 1, 1, c)
        near |= np.abs(e[c] - x) <= f32(2.0) * np.spacing(x)
    return int(np.count_nonzero(near))


def test_near_edge_photons_are_common_at_a_large_origin():
    count = near_edge_photons(4096.0)
    print("photons within two spacings of a forward edge, origin 4096:", count, "; origin 65536:", near_edge_photons(65536.0))
    assert count >= MIN_NEAR_EDGE
    assert near_edge_photons(0.0) < count


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_photons_near_an_edge_are_not_landed(place, tbl):
    assert near_edge_photons(4096.0) >= MIN_NEAR_EDGE                          # (the not-landed path runs)
    setting = ("3x5x7", 1.0)
    g = integrator(*setting, place, origin=4096.0)
    ref, spread = reference(g, place, setting, [EDGE_LAUNCH])
    assert ref[EDGE_LAUNCH]["counters"]["scatterings"] > 0      # (at this origin the tracer drops a few photons -- 21 of 4097 -- in every kernel alike)
    check(g, ref, spread, place, tbl, setting, [EDGE_LAUNCH], lambda launch: True)
    g.finalize_Integrator()


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_a_start_height_that_rounds_to_the_top_is_not_eligible(place, tbl):
    setting = ("3x5x7", 1.0)
    xe, ye, ze, _ = field("3x5x7", z0=4096.0)
    assert f32(ze[0] + (f32(1.0) - np.spacing(f32(1.0))) * f32(ze[-1] - ze[0])) == ze[-1]
    g = integrator(*setting, place, z0=4096.0)
    ref, spread = reference(g, place, setting, [EDGE_LAUNCH])
    check(g, ref, spread, place, tbl, setting, [EDGE_LAUNCH], lambda launch: False)
    g.finalize_Integrator()
