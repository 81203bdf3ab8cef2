"""The production photon streams against an independent float64 model (tests/stream_model.py) -- deterministic: the same seed and
photon numbers on both sides, integer work counters equal, every tally entry within the model's own propagated float32 bound.

What this pins that no other test does: the roles of an event's Philox block, the next() cursor on the photon's block counter, the
key's second word in fused launches, photon numbers beyond 2^32 where the kernels hand them out, the local estimate's own roulette
(the `r ...` cases: make_ray's second statement of the key rule and its tail, the service phase's stages and second leg, the ring record's
photon-high-or-batch word, the skipped rays and the tracer calls; a downward direction exactly 0), and the production arithmetic
(scattering_cosine<false>, next_direct's hardware branch, fast_log, the reflection from hardware sin / cos, lookup_phase_fast,
fast_div, fast_exp).  Every kernel shares those routines, so the kernel-against-kernel tests cannot see a mistake in them, and the
statistical tests see nothing below 1e-4 of a domain mean.

Each shared case (stream_model.CASES) runs once on the kernel the library chooses and once on the general kernel, and so does its
longest run of photons without a fragile one (there the float32 bound alone is allowed); nothing is run a second time.  A fragile photon (one whose discrete decisions the model cannot vouch for at float32 precision; at most 0.5 % of a
case, asserted on the CPU) may take another branch: the counters may differ by what the fragile photons count in the model, a
tally entry by the weight they carry.  Beyond that a difference is a finding: a wrong kernel, or a comment in tracer.hpp that
understates an approximation's error.

Measured on an MI355X (the module: 39 tests in 9 s): every counter of every run equal to the model's -- no fragile photon took another
branch --, and the largest tally difference as a fraction of the propagated float32 bound ALONE (kernel chosen | general; the figures
are the same for both, and for the whole case and its run without fragile photons to within a factor two):
  a common        flux, table in LDS | general flux       0 (sums of whole weights)     fragile share 0.0019
  a absorbing     flux, table in LDS | general flux       0.12                          0.0013
  b records       flux               | general flux       0.07                          0.0014
  c two, d three  general flux (both)                     0.18, 0.19                    0.0025, 0.0028
  e irregular     general flux (both)                     0.09                          0.0023
  f no roulette / roulette   flux, table in LDS | general 0.36 / 0.40                   0.0046 / 0.0003
  g black / white            flux, table in LDS | general 0.06 / 0.06                   0.0008 / 0.0044
  h one up / down / hybrid   radiance, one direction | general radiance, one direction  0.09 / 0.07 / 0.09   0.0027 / 0.0029 / 0.0032
  h three / limit            radiance (ring) | general radiance                         0.07 / 0.07          0.0033 / 0.0031
  h three two components     radiance, wide | general radiance                          0.20                 0.0047
  first photon 2^32 - 700, 2^33 + 5 (a, h three): 0, 0.09;  fused batches (PhiloxBatchStream: flux with the table in LDS; radiance, one direction): 0, 0.06
with the local estimate's roulette (the intensity's largest difference / float32 bound alone: whole case | its run without fragile photons;
the same on the kernel chosen and the general one; every counter -- raysSkipped and tracerCalls among them -- equal to the model's):
  r one up                   radiance, one direction | general ... | radiance (ring, kernel="ring")   0.04 | 0.07 (all three)   0.0021
  r one down                 radiance, one direction | general radiance, one direction               0 | 0 (exactly 0)        0.0014
  r three / r wide           radiance (ring) | general radiance                                      0.04 | 0.05 (both)       0.0023 / 0.0010
  r three two components     radiance, wide | general radiance                                       0.02 | 0.04              0.0023
  r hybrid                   radiance, one direction | general radiance, one direction               0.04 | 0.09              0.0024
  r limit                    radiance (ring) | general radiance     0.04 | 0.05, intensityExcess 0.006 | 0.024 (r wide: 0.008 | 0.008)   0.0021
  r zeta (zetaMin 1.5)       radiance (ring) | general radiance                                      0.06 | 0.12              0.0015
  first photon 2^32 - 700, 2^33 + 5 (r one up; r three): 0.05, 0.04; 0.06, 0.04;  fused batches (r one up: one direction; r three: the ring,
  whose record carries the batch in place of the photon's high word): 0.04, 0.04
  where only the float32 bound is allowed: the clean windows beyond 2^32 (468 and 848 photons; r one up; r three): 0.06, 0.06; 0.09, 0.04;
  fused batches 0, 1, 2 of S.FUSED_CLEAN_SEED, 750 photons each without a fragile one (r one up; r three): 0.04, 0.05, 0.06; 0.11, 0.04, 0.07,
  the group's counters equal to the models' sums"""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import stream_model as S
from tests.test_stream_model_cpu import beyond_two_to_the_32, model_for, tables

pytestmark = pytest.mark.gpu


def _integrator(name):
    c = S.CASES[name]
    p = c["params"]
    nz, ny, nx = len(c["ze"]) - 1, len(c["ye"]) - 1, len(c["xe"]) - 1
    dom = M.new_Domain(c["xe"], c["ye"], c["ze"])
    tabs = [tables(tuple(gs), bool(p.get("hybrid"))) for gs in c["gs"]]
    full = lambda a, t: np.ascontiguousarray(np.broadcast_to(np.asarray(a)[:, None, None], (nz, ny, nx))).astype(t)   # noqa: E731
    for k, gs in enumerate(c["gs"]):
        dom.addOpticalComponent(f"component {k + 1}", full(c["ext"][k], np.float32), full(c["ssa"][k], np.float32), full(c["pfi"][k], np.int32),
                                M.PhaseFunctionTable([M.henyey_greenstein(g, 8) for g in gs]))   # (stand-ins: the tables are handed over below)
    g = M.new_Integrator(dom)
    kw = dict(surfaceAlbedo=p["albedo"], useRussianRoulette=p.get("roulette", True))
    if "mus" in p:
        kw.update(intensityMus=p["mus"], intensityPhis=p["phis"], useRussianRouletteForIntensity=bool(p.get("rr_intensity")),
                  zetaMin=p.get("zeta_min", 0.3))
    if p.get("hybrid"):
        kw.update(useHybridPhaseFunsForIntenCalcs=True, numOrdersOrigPhaseFunIntenCalcs=int(p["hybrid"]))
    if "limit" in p:
        kw.update(limitIntensityContributions=True, maxIntensityContribution=p["limit"])
    g.specifyParameters(**kw)
    for k, (inv, fwd, orig) in enumerate(tabs):
        g.set_tables(k + 1, inverse=inv, **(dict(forward=fwd, forward_orig=orig) if "mus" in p else {}))
    if "mus" in p:
        assert np.array_equal(g.intensityDirections, S.case_directions(c))   # (the directions the model was given are the device's)
    return g


def _shaped(g, res, model):
    """a run's raw tallies in the model's shapes"""
    lay, raw = g.layout(), res["raw"]
    at = dict(fluxUp=lay.fluxUp, fluxDown=lay.fluxDown, fluxAbsorbed=lay.fluxAbsorbed, volumeAbsorption=lay.volumeAbsorption,
              intensity=lay.intensityByComponent, intensityExcess=lay.intensityExcess)
    return {k: raw[at[k]:at[k] + v.size].reshape(v.shape) for k, v in model.tallies.items()}


def _hold(g, res, model, what, counter_names=S.COUNTERS_EXACT + S.COUNTERS_FRAGILE):
    miss, worst = S.compare(model, _shaped(g, res, model), res["counters"], counter_names)
    alone = {}   # (for the record: against the propagated float32 bound alone, without what the fragile photons may carry)
    for k, got in _shaped(g, res, model).items():
        diff, bound = np.abs(got - model.tallies[k]), model.bounds[k]
        alone[k] = float(np.max(np.where(diff > 0, diff / np.where(bound > 0, bound, S.TINY), 0.0)))
    print(f"{what}: kernel {g.kernel_name()} fragile {model.fragile_share:.5f} largest difference / tolerance "
          + " ".join(f"{k} {v:.3g}" for k, v in worst.items()) + " | / float32 bound alone " + " ".join(f"{k} {v:.3g}" for k, v in alone.items()))
    assert miss == [], (what, g.kernel_name(), miss, model.per_photon["why"])
    for k, zero in model.exact_zero.items():   # (the roulette: a downward direction's field is exactly 0 -- S.compare allows those entries nothing)
        assert not _shaped(g, res, model)[k][zero].any(), (what, k)


def _differ(name):
    """does the library choose another kernel than the general one?  (tests/kernel_matrix.py: plain FLUX launches of the widened class
    -- several components, irregular x / y -- run the general flux kernel; everything else has a kernel of its own)"""
    c = S.CASES[name]
    widened = len(c["gs"]) > 1 or c["xe"] is not S._XE
    return "mus" in c["params"] or not widened


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_against_the_model(name):
    n = S.CASES[name]["n"]
    model = model_for(name)
    g = _integrator(name)
    p = S.CASES[name]["params"]
    if p.get("rr_intensity"):   # (the entries _hold asserts to be exactly 0 are the downward directions')
        down = [m < 0 for m in p["mus"]]
        assert [bool(model.exact_zero["intensity"][0, d].all()) for d in range(len(down))] == down
    names = []
    for kernel in ("auto", "general"):
        g.set_tuning(kernel=kernel)
        res = g.computeRadiativeTransfer(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, n))
        names.append(g.kernel_name())
        _hold(g, res, model, f"{name} [{kernel}]")
        # ... and the case's longest run of photons without a fragile one on its own: counters equal, tallies within the float32 bound alone
        first, count = S.clean_range(model)
        clean = model_for(name, first=first, n=count)
        assert count >= 500 and not clean.per_photon["fragile"].any()
        g.launch(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, count), firstPhoton=first)
        _hold(g, g.finish(), clean, f"{name} photons {first} .. {first + count - 1} [{kernel}]")
    assert ", true, GRID_" in names[1], names
    assert (names[0] != names[1]) == _differ(name), (name, names)
    nd = len(S.CASES[name]["params"].get("mus", ()))
    if nd:
        assert ("one direction" in names[0]) == (nd == 1), names
    g.finalize_Integrator()


def test_one_direction_through_the_event_ring():
    """the same photons of the one-direction roulette case through the event ring (make_ray in the EXPAND phase, from the event's record)
    instead of the event phase's registers: the whole case and its run without fragile photons"""
    name = "r one up"
    model = model_for(name)
    g = _integrator(name)
    g.set_tuning(kernel="ring")
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, S.CASES[name]["n"]))
    assert "one direction" not in g.kernel_name() and ", true, GRID_" not in g.kernel_name(), g.kernel_name()
    _hold(g, res, model, f"{name} [ring]")
    first, count = S.clean_range(model)
    g.launch(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, count), firstPhoton=first)
    _hold(g, g.finish(), model_for(name, first=first, n=count), f"{name} photons {first} .. {first + count - 1} [ring]")
    g.finalize_Integrator()


@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["a common", "h three", "r one up", "r three"])
def test_photon_numbers_across_two_to_the_32(name, first):
    n = 1500
    model = model_for(name, first=first, n=n)
    g = _integrator(name)
    for kernel in ("auto", "general"):
        g.set_tuning(kernel=kernel)
        g.launch(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, n), firstPhoton=first)
        _hold(g, g.finish(), model, f"{name} first photon {first} [{kernel}]")
        if S.CASES[name]["params"].get("rr_intensity"):
            # ... and the longest run without a fragile photon among the photons whose number has a high word, on its own: there a ray
            # block keyed without that word (the ring record's) fails the comparison (tests/test_stream_model_cpu.py)
            at, count = beyond_two_to_the_32(name, first, n)
            clean = model_for(name, first=at, n=count)
            assert at >= 2 ** 32 and count >= 150 and not clean.per_photon["fragile"].any()
            g.launch(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, count), firstPhoton=at)
            _hold(g, g.finish(), clean, f"{name} photons {at} .. {at + count - 1} [{kernel}]")
    g.finalize_Integrator()


def _fused_kernel_is_the_one_meant(g, name):
    """one direction: the kernel without a ring; more: the ring kernel, whose record carries the batch in place of the photon's high
    word -- and never the general kernel"""
    nd = len(S.CASES[name]["params"].get("mus", ()))
    assert ", true, GRID_" not in g.kernel_name() and ("one direction" in g.kernel_name()) == (nd == 1), g.kernel_name()
    assert ("PhiloxBatchStream, true, false" in g.kernel_name()) == (nd > 0), g.kernel_name()


@pytest.mark.parametrize("name", S.FUSED_CLEAN_CASES)
def test_fused_batches_without_a_fragile_photon(name):
    """A fused launch where nothing but the float32 bound is allowed: S.FUSED_CLEAN_N photons a batch of the key S.FUSED_CLEAN_SEED, whose
    batches 0, 1 and 2 hold no fragile photon.  Every batch's tallies within the bound alone, the group's counters equal: a ray key
    without `+ batch`, or a ring record that loses its batch word, fails exactly this (tests/test_stream_model_cpu.py)."""
    n, nb = S.FUSED_CLEAN_N, 3
    g = _integrator(name)
    g.set_batch_fusion(1)
    rs = g.computeRadiativeTransferBatches(S.FUSED_CLEAN_SEED, nb, *S.SUN, n)
    assert g.last_plan()["fusedBatches"] == nb and "PhiloxBatchStream" in g.kernel_name(), (g.last_plan(), g.kernel_name())
    _fused_kernel_is_the_one_meant(g, name)
    models = [model_for(name, seed=S.FUSED_CLEAN_SEED, n=n, batch=b) for b in range(nb)]
    assert not any(m.per_photon["fragile"].any() for m in models)
    for b in range(nb):
        _hold(g, rs[b], models[b], f"{name} fused batch {b} without fragile photons", S.COUNTERS_EXACT)
    total = {k: sum(r["counters"][k] for r in rs) for k in S.COUNTERS_EXACT + S.COUNTERS_FRAGILE}
    assert S.compare_counters(models, total) == [], (S.compare_counters(models, total), total)   # (no fragile photon: no allowance)
    g.finalize_Integrator()


@pytest.mark.parametrize("name", ["a common", "h one up", "r one up", "r three"])
def test_fused_batches(name):
    n, nb = S.CASES[name]["n"], 3
    g = _integrator(name)
    g.set_batch_fusion(1)
    rs = g.computeRadiativeTransferBatches(S.SEED, nb, *S.SUN, n)
    assert g.last_plan()["fusedBatches"] >= 2 and "PhiloxBatchStream" in g.kernel_name(), (g.last_plan(), g.kernel_name())
    _fused_kernel_is_the_one_meant(g, name)
    models = [model_for(name, seed=(S.SEED[0], S.SEED[1] + b)) for b in range(nb)]
    # (a fused RADIANCE launch counts photons and dropped photons per batch and its other work per wave, over the group: photon_kernel
    # -- flush_counters hands the wave's skipped rays to the batch in hand like the rest)
    per_batch = S.COUNTERS_EXACT if "mus" in S.CASES[name]["params"] else S.COUNTERS_EXACT + S.COUNTERS_FRAGILE
    for b in range(nb):
        _hold(g, rs[b], models[b], f"{name} fused batch {b}", per_batch)
    total = {k: sum(r["counters"][k] for r in rs) for k in S.COUNTERS_EXACT + S.COUNTERS_FRAGILE}
    assert S.compare_counters(models, total) == [], (S.compare_counters(models, total), total)
    g.finalize_Integrator()
