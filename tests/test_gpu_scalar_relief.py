"""What the event phase and the photon step of the specialised flux kernels of plain launches (photon_kernel, STORE; csrc/kernels.hpp,
csrc/tracer.hpp) ask the launch instead of working it out per phase: "can play roulette" as the bit kPlaysRoulette of
DevProblem::eventFlags, made on the host, and the step's face masks as `quotient <= advance` (trace_step_lazy,
STEP_ADVANCE_MASKS).  None of that may show: on every case each of the six kernels -- the field in LDS, in global memory read linearly
and as column records, each without and with the inverse table in LDS -- gives what the general flux kernel gives on the same launch:
all eleven counters and every word of the raw tally buffer with `==`.

The cases are chosen for the arms the change touches:
  domains   1 x 1 x 1 (optical depth 0.3), 3 x 5 x 7 (every column its own extinction, optical depth 0.6 ... 2.4) and 32 x 1 x 16
            (optical depth 2 | 18 in its two halves); every column holds one value over all its layers, which is a field all three
            places of the field can hold;
  photons   1, 63, 64, 65 (a wavefront less one lane, exactly, and one lane alone in a second wave), 4097;
  roulette  useRussianRoulette off and on, surface albedo 0 and 0.5, single-scattering albedo 1 and 0.5: all four values of
            (kWeightStaysOne, kPlaysRoulette), a scattering that ends a photon by roulette, a reflection that goes on.  0.5, so that a
            weight is a power of two and the roulette resets it to 0 or 1;
  sun       at the zenith (direction cosines of exactly 0: the step's NaN rule beside the new masks) and at mu0 = 0.5, azimuth 40 degrees;
  last interval   scattering_cosine's other arm, a deviate in the inverse table's last interval, which the six kernels read from LDS or
            from global memory: with a table of SHORT_TABLE angles on the 32 x 1 x 16 domain a sixteenth of the scattering deviates takes
            it.  How many do is counted on the CPU first, from Philox alone (test_the_short_table_reaches_its_last_interval).
Nothing here tries to provoke a fault; `dropped` is compared like every other counter.

Where `==` holds for the tally words.  With the roulette on, or without absorption, a weight is one of a few powers of two near 1 and
every float64 sum is exact in any order.  With omega = 0.5 and the roulette OFF (weights_only_halve) a weight halves at every scattering
and every reflection, down to 2^-126, and a float64 sum of such addends can depend on the order in which the atomics arrive.  Two rules
decide each such launch, in this order:
  provably exact   every addend is 2^-j with j <= J = scatterings + surfaceHits + 1 of the WHOLE launch (no photon has more events than the
            launch), so every partial sum is a multiple of 2^-J; no tally word exceeds 2 photons (a photon adds less than 2 to any tally);
            with J + log2(2 photons) <= 53 every partial sum fits a float64: `==`, and the general kernel's reruns must agree too;
  the reference's own reruns   otherwise the general kernel runs the launch three times.  Reruns equal word for word: `==`.  Reruns that differ
            show the launch to depend on the order (32 x 1 x 16 with 4097 photons: some 50 ... 100 words, by 1 ... 4 units of the last
            place): there a word may differ from the reference by four times the largest relative difference among the reference's own
            runs, which itself must stay below 16 * 2^-52.
The counters are compared with `==` on every launch."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from i3rc_monte_carlo_model_amd import binding as B
from tests import stream_model as S
from tests.philox_ref import philox4x32_10
from tools import record_event_bookkeeping as R

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = (43, 7)
PHOTONS = (1, 63, 64, 65, 4097)
SHAPES = {"1x1x1": (1, 1, 1), "3x5x7": (3, 5, 7), "32x1x16": (32, 1, 16)}
SSAS = (1.0, 0.5)
ALBEDOS = (0.0, 0.5)
ROULETTES = (False, True)
SUNS = ((1.0, 0.0), (0.5, 40.0))
SHORT_TABLE = 16                                        # angles of the short inverse table
LAST = ("32x1x16", 1.0, "short")                        # domain, single-scattering albedo, table of the last-interval case
LAST_LAUNCH = (0.0, False, PHOTONS[-1], SUNS[0])        # ... and its surface albedo, roulette, photons, sun
IDS = [f"{p}{' table in LDS' if t else ''}" for p, t in R.KERNELS]


def settings():
    """(domain, single-scattering albedo, table) of every integrator at one place of the field"""
    return [(which, ssa, "hg") for which in SHAPES for ssa in SSAS] + [LAST]


def launches(setting):
    """(surface albedo, roulette, photons, sun) of every launch on one integrator"""
    if setting == LAST:
        return [LAST_LAUNCH]
    return [(a, rr, n, sun) for a in ALBEDOS for rr in ROULETTES for n in PHOTONS for sun in SUNS]


RERUNS = 3                                              # runs of the general kernel where a launch's sums may depend on the order


def weights_only_halve(setting, launch):
    """absorption and no roulette: weights that halve without end (see the module's text)"""
    return setting[1] == 0.5 and not launch[1]


def provably_exact(launch, counters):
    """every partial sum of every tally word of the launch fits a float64 (see the module's text)"""
    return counters["scatterings"] + counters["surfaceHits"] + 1 + np.log2(2.0 * launch[2]) <= 53


def spread_of(runs):
    """largest relative difference of a word among runs of one launch; 0.0: equal word for word"""
    worst = 0.0
    for i in range(len(runs)):
        for j in range(i):
            bad = runs[i] != runs[j]
            if bad.any():
                worst = max(worst, float((np.abs(runs[i] - runs[j])[bad] / np.maximum(np.abs(runs[i][bad]), np.abs(runs[j][bad]))).max()))
    return worst


def optical_depths(which):
    nx, ny, _ = SHAPES[which]
    n = nx * ny
    if which == "1x1x1":
        return np.full(n, f32(0.3))
    if which == "3x5x7":
        return f32(0.6) + f32(1.8) * np.arange(n, dtype=f32) / f32(n - 1)
    return np.where(np.arange(n) < n // 2, f32(2.0), f32(18.0)).astype(f32)


def short_table():
    """SHORT_TABLE scattering angles, ascending from 0 to pi: an inverse table as the device takes it (any ascending angles are one)"""
    return (f32(np.pi) * np.arange(SHORT_TABLE, dtype=f32) / f32(SHORT_TABLE - 1)).astype(f32)


def integrator(setting, place):
    which, ssa, table = setting
    nx, ny, nz = SHAPES[which]
    ze = (np.arange(nz + 1, dtype=f32) / f32(nz)).astype(f32)                  # layers of equal depth, 1 in all
    ext = np.broadcast_to(optical_depths(which).reshape(1, ny, nx), (nz, ny, nx)).astype(f32)   # (extinction = optical depth)
    dom = M.new_Domain((f32(0.25) * np.arange(nx + 1)).astype(f32), (f32(0.25) * np.arange(ny + 1)).astype(f32), ze)
    dom.addOpticalComponent("cloud", ext, np.full(ext.shape, f32(ssa)), np.ones(ext.shape, np.int32),
                            M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]))
    g = M.new_Integrator(dom)
    if table == "short":
        g.set_tables(1, inverse=short_table())
    g.select_grid_place(R.KNOB[place])
    return g


def run(g, kernel, launch):
    albedo, roulette, photons, sun = launch
    g.specifyParameters(surfaceAlbedo=albedo, useRussianRoulette=roulette)
    g.set_tuning(kernel=kernel)
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*sun, photons), firstPhoton=0)
    res = g.finish()
    return res, g.kernel_name()


@pytest.fixture(scope="module")
def general():
    """per place of the field and setting: the integrator (shared with the tests, which only launch on it), the general kernel's
    result of every launch, and, where weights only halve, the spread of the general kernel's own RERUNS runs of the launch: computed
    once, never written to"""
    out = {}
    for place in ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS"):
        for setting in settings():
            g = integrator(setting, place)
            ref, spread = {}, {}
            for launch in launches(setting):
                res, name = run(g, "general", launch)
                assert name == R.kernel_name(place, False, True), name
                res["raw"].setflags(write=False)
                ref[launch] = res
                if weights_only_halve(setting, launch):
                    again = [run(g, "general", launch)[0] for _ in range(RERUNS - 1)]
                    assert all(a["counters"] == res["counters"] for a in again), (place, setting, launch)
                    spread[launch] = spread_of([res["raw"]] + [a["raw"] for a in again])
            out[place, setting] = (g, ref, spread)
    yield out
    for g, _, _ in out.values():
        g.finalize_Integrator()


def last_interval_scatterings():
    """A lower bound, from Philox alone, of the scatterings of the last-interval launch whose deviate falls into the table's last
    interval.  Under a sun at the zenith a photon goes straight down from the top, and every column is at least 2 deep: with a first
    optical depth below 1.9 -- path(), word 2 of the photon's block 0 -- its first event is a scattering, whose angle deviate is
    first(), word 0 of its block 1 (philox.hpp, the roles above PhiloxStreamT).  The interval as the kernels find it, in float32:
    k = int(r * n) + 1 >= n, which is what r in [1 - 1 / n, 1] comes to."""
    n = LAST_LAUNCH[2]
    pid = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, np.uint64)
    start = S.philox(pid, zero, 0, 0, SEED[0], SEED[1])
    event = S.philox(pid, zero, 1, 0, SEED[0], SEED[1])
    assert tuple(int(w[n - 1]) for w in event) == philox4x32_10((n - 1, 0, 1, 0), SEED)   # (the array form against the scalar one)
    tau = -np.log(np.maximum(np.finfo(f32).tiny, S.unit(start[2])))
    r = S.unit(event[0]).astype(f32)
    k = (r * f32(SHORT_TABLE)).astype(f32).astype(np.int64) + 1
    return int(np.count_nonzero((tau < 1.9) & (k >= SHORT_TABLE)))


def test_the_short_table_reaches_its_last_interval(general):
    count = last_interval_scatterings()
    print("scatterings in the last interval of the short table, at least:", count)
    assert count >= 10
    for place in ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS"):
        assert general[place, LAST][1][LAST_LAUNCH]["counters"]["scatterings"] >= count


def test_where_the_sums_depend_on_the_order(general):
    """the two rules of the module's text, on the reference alone: a provably exact launch reruns equal, one photon always does (its
    addends arrive in its own order), and a spread stays within a few units of the last place"""
    seen = {"provably exact": 0, "reruns equal": 0, "reruns differ": 0}
    for (place, setting), (_, ref, spread) in general.items():
        for launch, s in spread.items():
            what = (place, setting, launch, s)
            if provably_exact(launch, ref[launch]["counters"]) or launch[2] == 1:
                assert s == 0.0, what
            assert s <= 16 * 2.0 ** -52, what
            seen["provably exact" if provably_exact(launch, ref[launch]["counters"]) else ("reruns equal" if s == 0.0 else "reruns differ")] += 1
    print("launches whose weights only halve:", seen)
    assert seen["provably exact"] > 0


def test_the_cases_reach_the_arms(general):
    """every photon is accounted for; a roulette is played exactly where the launch can play one and weights fall below a half; without
    absorption over a black surface nothing is absorbed and every photon ends at a boundary"""
    for (place, setting), (_, ref, _) in general.items():
        which, ssa, _ = setting
        for launch, res in ref.items():
            albedo, roulette, photons, sun = launch
            n = res["counters"]
            what = (place, setting, launch, n)
            assert n["photons"] == photons, what
            assert n["tracerCalls"] == n["scatterings"] + n["surfaceHits"] + n["exitsTop"] + n["dropped"], what
            stays_one = ssa == 1.0 and albedo == 0.0
            if not roulette or stays_one:
                assert n["roulette"] == 0, what
            if stays_one:
                assert n["surfaceHits"] + n["exitsTop"] + n["dropped"] == photons, what
            if photons == PHOTONS[-1]:
                assert n["scatterings"] > 0 and n["exitsTop"] > 0 and n["surfaceHits"] > 0, what
                if roulette and ssa == 0.5 and which != "1x1x1":
                    assert n["roulette"] > 0, what            # (two scatterings bring a weight to 0.25)
                if albedo == 0.5:
                    assert n["surfaceHits"] + n["exitsTop"] > photons or ssa == 0.5, what   # (a reflection went on)


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_equals_general_kernel(place, tbl, general):
    for setting in settings():
        g, ref, spread = general[place, setting]
        for launch in launches(setting):
            got, name = run(g, "auto" if tbl else "lane", launch)
            want = ref[launch]
            what = (place, tbl, setting, launch)
            assert name == R.kernel_name(place, tbl), (what, name)
            assert sorted(got["counters"]) == sorted(B.COUNTER_NAMES), what
            for k in B.COUNTER_NAMES:
                assert got["counters"][k] == want["counters"][k], (what, k, got["counters"], want["counters"])
            assert got["raw"].shape == want["raw"].shape, what
            if spread.get(launch, 0.0) > 0.0 and not provably_exact(launch, want["counters"]):   # (the reference's own reruns differ)
                off = np.abs(got["raw"] - want["raw"]) > 4.0 * spread[launch] * np.abs(want["raw"])
                assert not off.any(), (what, spread[launch], np.flatnonzero(off))
            else:
                assert (got["raw"] == want["raw"]).all(), (what, np.flatnonzero(got["raw"] != want["raw"]))
