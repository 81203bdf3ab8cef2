"""The float64 stream model (tests/stream_model.py) is right on its own, and its tolerances would catch a subtly wrong kernel --
both shown without a GPU:

  * Philox known answers (Random123's kat_vectors for philox4x32-10) for tests/philox_ref.py and the model's vectorised form;
  * the model against the adding-doubling solver on the cases of tests/test_plane_parallel.py, 4 standard errors of its own sample;
  * the model against the CPU oracle on a two-component layered case with a reflecting surface and a radiance direction
    (two independent samples: combined standard errors);
  * the share of fragile photons of every shared case, asserted below 0.5 % (a condition on the inputs);
  * energy: up + absorbed + (1 - albedo) down = 1 per photon without roulette;
  * the controls: a model that swaps first() and second(), takes the azimuth from first(), interpolates the inverse table one
    interval on, or drops the high word of the photon number must FAIL the comparison the GPU module makes, at the shared cases' sizes;
  * the local estimate's own roulette (the `r ...` cases): the model with it against the solver and the oracle (a downward direction
    exactly 0 on both sides); every branch a ray can take holds 200 rays over the cases and 20 inside their runs without a fragile
    photon; and its controls -- a ray block that ignores the direction number, d instead of d + 1 in the fourth counter word, r2 from
    word 0, a fused ray key without the batch, a second leg restarted at the event, a downward direction that counts -- FAIL the
    comparison on the run without fragile photons, and on a whole case where one can see them at all (RAY_CONTROLS says which, and why
    a mere re-draw of the rays' deviates is a thousandth of what a whole case allows its fragile photons).  A fused launch starts at
    photon 0: the key S.FUSED_CLEAN_SEED, whose three batches begin with 750 photons none of them fragile, is where the key without
    the batch fails for fused launches; a ray block without the photon's high word fails on the clean window beyond 2^32;
  * the four diagnostic tallies (Problem.extra: levels, tracks, paths, bins), compared over photons that are not fragile only:
    identities exact in the model's float64, per photon and per column (levelFluxDown[0] = fluxDown, levelFluxUp[nz] = fluxUp, the
    sum of levelFluxDown[nz] = n, the bins add up to the fluxes and the path bins to the first moments, the cells' track lengths to
    the photons' w |s|; without roulette the net level flux into a layer is what the photon leaves there, to 1e-12); batches of the
    model against tests/level_flux_solver.py at every level, against the equivalence-theorem figures of tests/test_gpu_path_lengths.py
    (+ the reference's own finite-difference uncertainty) and (1 - omega) sigma dz <actinic flux> against the net-flux divergence, 4
    standard errors + SOLVER; the conditions on the inputs -- fragile shares with the new decisions within the cap for every case and
    kind (S.DIAGNOSTIC_SHARES), histogram edges per case with an overflow bin that holds something but under 1 % of the weight, 20 bins
    of 100 photons and no edge within 1e-4 of the unscattered path, track bounds at most 1e-3 of every cell with 1000 pieces --; and
    eleven controls (S.EXTRA_VARIANTS), each FAILING the GPU module's comparison on `a absorbing` and on `c two` by the diagnostic
    fields alone."""
import functools

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import stream_model as S
from tests.philox_ref import philox4x32_10

N_TABLE = 9001
# the adding-doubling solver's own error (tests/test_plane_parallel.py::test_the_solver_itself holds its energy balance and its convergence
# in the number of streams to this): what a quantity with no sampling error at all -- the absorption of a conservative slab, exactly 0
# in the model, 1.6e-8 in the solver -- may differ by
SOLVER = 1e-6


@functools.lru_cache(maxsize=None)
def _hg(g):
    return M.henyey_greenstein(g, 299 if g >= 0.9 else (64 if g > 0.7 else 32))


@functools.lru_cache(maxsize=None)
def tables(gs, hybrid=False):
    """(inverse, forward in use, original forward) of one component's table, as the host makes them"""
    t = M.PhaseFunctionTable([_hg(g) for g in gs])
    inv, orig = t.inverse_table(N_TABLE), t.forward_table(N_TABLE)
    fwd = M.phasefunctions.hybrid_phase_functions(orig, 7.0) if hybrid else orig
    return np.asarray(inv, np.float32), np.asarray(fwd, np.float32), np.asarray(orig, np.float32)


def case_problem(name):
    c = S.CASES[name]
    tabs = [tables(tuple(gs), bool(c["params"].get("hybrid"))) for gs in c["gs"]]
    return S.problem(c, [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], S.case_directions(c))


@functools.lru_cache(maxsize=None)
def model_for(name, seed=S.SEED, first=0, n=None, variant=None, drop=False, batch=0):
    return S.run(case_problem(name), seed, first, n or S.CASES[name]["n"], variant=variant, drop_high_word=drop, batch=batch)


def diagnostic_problem(name, kind):
    """the model's problem for the shared flux case `name` with the diagnostic tally `kind` on (S.diagnostic_case: its own columns, or wide ones)"""
    c = S.diagnostic_case(name, kind)
    return S.problem(c, [tables(tuple(gs))[0] for gs in c["gs"]], extra=kind, bin_edges=S.bin_edges(name) if kind == "bins" else None)


@functools.lru_cache(maxsize=None)
def diagnostic_model(name, kind, first=None, n=None, variant=None):
    """the whole case (first: the first photon, by default the kind's and case's own -- S.DIAGNOSTIC_FIRST, else 0)"""
    first = S.DIAGNOSTIC_FIRST.get((kind, name), 0) if first is None else first
    return S.run(diagnostic_problem(name, kind), S.SEED, first, n or S.CASES[name]["n"], variant=variant)


def diagnostic_runs(name, kind, first=None, n=None, start=0, least=1):
    """every maximal run (first photon, count) of at least `least` photons of the case none of which is fragile -- with the kind's own
    decisions among the reasons --, as photon numbers: what the GPU module launches one after the other into one block"""
    first = S.DIAGNOSTIC_FIRST.get((kind, name), 0) if first is None else first
    return [(first + a, c) for a, c in S.clean_runs(diagnostic_model(name, kind, first, n), start=start, least=least)]


@functools.lru_cache(maxsize=None)
def diagnostic_clean(name, kind, variant=None, first=None, n=None, start=0, least=1):
    """the model over exactly the photons of diagnostic_runs: the expected value of every diagnostic entry, with the float32 bound alone"""
    return S.run(diagnostic_problem(name, kind), S.SEED, 0, 0, variant=variant, ids=S.run_ids(diagnostic_runs(name, kind, first, n, start, least)))


# ---- Philox ----------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert philox4x32_10(ctr, key) == want
        assert tuple(int(v) for v in S.philox(*ctr, *key)) == want
    # ... and the vectorised form on arrays, against the scalar one
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, (4, 50), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
    out = np.array(S.philox(*c, *k))
    for i in range(50):
        assert tuple(int(v) for v in out[:, i]) == philox4x32_10(tuple(int(v) for v in c[:, i]), tuple(int(v) for v in k))


def test_deviate_mapping_reaches_both_ends():
    u = S.unit(np.array([0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64))
    assert u[0] == 0.0 and u[-1] == 1.0 and np.all(np.diff(u) >= 0) and u[2] == 0.5


# ---- against the solver ---------------------------------------------------------------------------------------------------------
def _slab(tau, omega, albedo, moments, dirs=None, n_table=10001, rr_intensity=False):
    from tools import cases

    d = cases.plane_parallel(optical_depth=tau, ssa=omega, nx=2, ny=2, nlayers=3)
    t = M.PhaseFunctionTable([M.henyey_greenstein(0.85, moments)])
    fwd = [t.forward_table(n_table)] if dirs is not None else None
    return S.Problem(d["xe"], d["ye"], d["ze"], d["ext"][:, 0, 0], d["ssa"][:, 0, 0], d["pf"][:, 0, 0], [t.inverse_table(n_table)],
                     mu0=0.5, azimuth=0.0, albedo=albedo, roulette=True, dirs=dirs, fwd=fwd, rr_intensity=rr_intensity)


def _means(results, key, axes):
    per = np.array([r.tallies[key].sum(axis=axes) / r.n for r in results])
    return per.mean(0), per.std(0, ddof=1) / np.sqrt(len(per))


@pytest.mark.parametrize("tau", [0.1, 1.0, 10.0])
@pytest.mark.parametrize("omega", [1.0, 0.9])
@pytest.mark.parametrize("albedo", [0.0, 0.5])
def test_model_fluxes_against_adding_doubling(tau, omega, albedo):
    from tests.plane_parallel_solver import solve
    from tests.test_plane_parallel import G, MOMENTS, MU0, _sampled_moments

    n, nb = (60_000 if tau < 5 else 20_000), 10          # (the sample of tests/test_plane_parallel.py's CPU runs)
    P = _slab(tau, omega, albedo, MOMENTS)
    rs = [S.run(P, (10, b), 0, n) for b in range(1, nb + 1)]
    want = solve(tau, omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    for key in ("fluxUp", "fluxDown", "fluxAbsorbed"):
        got, se = _means(rs, key, (0, 1))
        assert abs(got - want[key]) <= 4.0 * se + SOLVER, (key, tau, omega, albedo, got, want[key], se)


def _radiances_against_adding_doubling(tau, omega, albedo, rr_intensity):
    from tests.plane_parallel_solver import solve
    from tests.test_plane_parallel import G, MOMENTS_RADIANCE, MU0, VIEW_MUS, VIEW_PHIS

    n, nb = (60_000 if tau < 5 else 20_000), 10
    dirs = np.array([S.direction(m, p) for m, p in zip(VIEW_MUS, VIEW_PHIS)])
    P = _slab(tau, omega, albedo, MOMENTS_RADIANCE, dirs, rr_intensity=rr_intensity)
    rs = [S.run(P, (10, b), 0, n) for b in range(1, nb + 1)]
    want = solve(tau, omega, G, MU0, albedo=albedo, radiance_mus=VIEW_MUS, radiance_dphis_deg=VIEW_PHIS)
    per = np.array([r.tallies["intensity"].sum(axis=(0, 2, 3)) / r.n for r in rs])   # (mean over columns of sum / photons per column)
    got, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(nb)
    for k in range(len(VIEW_MUS)):
        assert abs(got[k] - want["intensity"][k]) <= 4.0 * se[k] + SOLVER, (k, tau, omega, albedo, got[k], want["intensity"][k], se[k])


RADIANCE_SLABS = [(1.0, 1.0, 0.0), (10.0, 0.9, 0.5), (0.1, 1.0, 0.5)]


@pytest.mark.parametrize("tau,omega,albedo", RADIANCE_SLABS)
def test_model_radiances_against_adding_doubling(tau, omega, albedo):
    _radiances_against_adding_doubling(tau, omega, albedo, False)


@pytest.mark.parametrize("tau,omega,albedo", RADIANCE_SLABS)
def test_model_radiances_with_the_roulette_against_adding_doubling(tau, omega, albedo):
    """the local estimate's roulette is unbiased: the solver's answer is the same, the rule is the same"""
    _radiances_against_adding_doubling(tau, omega, albedo, True)


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
def test_model_against_the_oracle_two_components_surface_radiance():
    from oracle import pyoracle as O

    O.build()
    name = "h three two components"
    c, P = S.CASES[name], case_problem(name)
    nz, ny, nx = len(c["ze"]) - 1, len(c["ye"]) - 1, len(c["xe"]) - 1
    full = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a)[:, :, None, None], a.shape + (ny, nx)))   # noqa: E731
    o = O.Integrator(c["xe"], c["ye"], c["ze"], full(c["ext"]).astype(np.float32), full(c["ssa"]).astype(np.float32),
                     full(c["pfi"]).astype(np.int32), P.inv, P.fwd, P.fwd_orig)
    p = c["params"]
    o.specify(surfaceAlbedo=p["albedo"], intensityMus=p["mus"][:1], intensityPhis=p["phis"][:1])
    P.dirs = P.dirs[:1]
    n, nb = 20_000, 10
    ors, ms = [], []
    for b in range(1, nb + 1):
        rng = O.RandomNumberSequence([10, b])
        ors.append(o.compute(rng, *O.photons_directional(rng, *S.SUN, n)))
        ms.append(S.run(P, (10, b), 0, n))
    for key in ("fluxUp", "fluxDown", "fluxAbsorbed", "intensity"):
        a = np.array([r[key].astype(np.float64).mean() for r in ors])
        m = np.array([(r.tallies[key].sum(0) if key == "intensity" else r.tallies[key]).sum() / r.n for r in ms])
        se = np.sqrt(a.var(ddof=1) / nb + m.var(ddof=1) / nb)
        assert abs(a.mean() - m.mean()) <= 4.0 * se, (key, a.mean(), m.mean(), se)


def test_model_against_the_oracle_with_the_roulette_up_and_down():
    """the same with the local estimate's roulette on both sides, an upward and a downward direction: the downward one's field is
    exactly 0 on both sides (only an exit through the top counts), the upward one's agrees within the two samples' errors"""
    from oracle import pyoracle as O

    O.build()
    name = "r three two components"
    c, P = S.CASES[name], case_problem(name)
    nz, ny, nx = len(c["ze"]) - 1, len(c["ye"]) - 1, len(c["xe"]) - 1
    full = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a)[:, :, None, None], a.shape + (ny, nx)))   # noqa: E731
    o = O.Integrator(c["xe"], c["ye"], c["ze"], full(c["ext"]).astype(np.float32), full(c["ssa"]).astype(np.float32),
                     full(c["pfi"]).astype(np.int32), P.inv, P.fwd, P.fwd_orig)
    p = c["params"]
    assert p["mus"][1] > 0 > p["mus"][2]
    o.specify(surfaceAlbedo=p["albedo"], intensityMus=p["mus"][1:], intensityPhis=p["phis"][1:], useRRForIntensity=1, zetaMin=P.zeta_min)
    P.dirs = P.dirs[1:]
    n, nb = 20_000, 10
    ors, ms = [], []
    for b in range(1, nb + 1):
        rng = O.RandomNumberSequence([10, b])
        ors.append(o.compute(rng, *O.photons_directional(rng, *S.SUN, n)))
        ms.append(S.run(P, (10, b), 0, n))
    assert all(not r["intensity"][1].any() for r in ors) and all(not r.tallies["intensity"][:, 1].any() for r in ms)
    assert sum(r.branches["second leg counted"] for r in ms) > 1000 and sum(r.branches["small won counted"] for r in ms) > 1000
    for key in ("fluxUp", "fluxDown", "fluxAbsorbed", "intensity"):
        a = np.array([(r[key][0] if key == "intensity" else r[key]).astype(np.float64).mean() for r in ors])
        m = np.array([(r.tallies[key][:, 0].sum(0) if key == "intensity" else r.tallies[key]).sum() / r.n for r in ms])
        se = np.sqrt(a.var(ddof=1) / nb + m.var(ddof=1) / nb)
        assert a.mean() > 0 and abs(a.mean() - m.mean()) <= 4.0 * se, (key, a.mean(), m.mean(), se)


# ---- the inputs: few fragile photons --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_fragile_share_of_the_shared_cases(name):
    r = model_for(name)
    assert r.fragile_share <= S.FRAGILE_CAP, (name, r.fragile_share, r.per_photon["why"])
    assert r.counters["scatterings"] > 0 and r.counters["surfaceHits"] > 0 and r.counters["exitsTop"] > 0
    assert abs(r.fragile_share - S.FRAGILE_SHARES[name]) < 1e-9, (name, r.fragile_share)   # (the shares written down are the ones measured)


@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["a common", "h three", "r one up", "r three"])
def test_fragile_share_across_two_to_the_32(name, first):
    assert model_for(name, first=first, n=1500).fragile_share <= S.FRAGILE_CAP


def test_energy_without_roulette():
    P = case_problem("f no roulette")
    r = S.run(P, S.SEED, 0, 5000)
    up, absorbed, down = (r.caps[k] - 1.0 for k in ("fluxUp", "fluxAbsorbed", "fluxDown"))   # (a cap is 1 + the photon's own deposit)
    per = up + absorbed + (1.0 - float(np.float32(P.albedo))) * down
    assert np.max(np.abs(per - 1.0)) < 1e-12, np.max(np.abs(per - 1.0))


# ---- the controls ---------------------------------------------------------------------------------------------------------------
def _fails(base, other):
    miss, worst = S.compare(base, other.tallies, other.counters)
    return len(miss) > 0


def clean_model(name, variant=None):
    """the model on the case's longest run of photons without a fragile one (what the GPU module launches on its own)"""
    first, count = S.clean_range(model_for(name))
    return model_for(name, first=first, n=count, variant=variant)


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_has_a_long_run_without_a_fragile_photon(name):
    r = clean_model(name)
    # (some hundreds of photons: every kind of event many times over)
    assert r.n >= 500 and not r.per_photon["fragile"].any(), (name, r.n)
    assert min(r.counters[k] for k in ("scatterings", "surfaceHits", "exitsTop")) >= 50, (name, r.counters)


@pytest.mark.parametrize("variant", S.VARIANTS[:2])
@pytest.mark.parametrize("name", ["a common", "c two", "h three"])
def test_a_changed_role_fails_the_comparison(name, variant):
    """first() and second() exchanged; the azimuth from first(): other photons altogether"""
    base = model_for(name)
    miss, _ = S.compare(base, base.tallies, base.counters)
    assert miss == []
    assert _fails(base, model_for(name, variant=variant)), (name, variant)
    assert _fails(clean_model(name), clean_model(name, variant)), (name, variant)


@pytest.mark.parametrize("name", ["h one up", "h one down", "h three", "h three two components", "h hybrid", "h limit"])
def test_the_next_table_interval_fails_the_comparison(name):
    """The inverse table read one interval on turns every scattering by about 1e-4 rad.  That moves no photon across a column's
    side at these sizes -- the flux tallies of the flux cases are sums of the same weights in the same entries (measured: `a common`,
    `c two`: not one entry differs) -- but every radiance contribution by about 1e-3 of itself, a thousand float32 bounds: the
    radiance cases see it, on the run without fragile photons, where nothing but the float32 bound is allowed."""
    assert _fails(clean_model(name), clean_model(name, S.VARIANTS[2])), name


@pytest.mark.parametrize("name", ["a common", "h three", "r three"])
@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
def test_a_dropped_high_word_fails_the_comparison(name, first):
    base = model_for(name, first=first, n=1500)
    assert _fails(base, model_for(name, first=first, n=1500, drop=True)), (name, first)


# ---- the local estimate's own roulette ------------------------------------------------------------------------------------------
RR_CASES = [k for k, c in S.CASES.items() if c["params"].get("rr_intensity")]


def test_the_roulette_cases_are_the_ones_asked_for():
    p = {k: S.CASES[k]["params"] for k in RR_CASES}
    nd = sorted(len(q["mus"]) for q in p.values())
    assert nd.count(1) >= 3 and nd.count(3) >= 2 and all(S.CASES[k]["n"] == 10_000 for k in RR_CASES)
    assert any(len(q["mus"]) == 1 and q["mus"][0] < 0 for q in p.values()) and any(q.get("hybrid") == 1 for q in p.values())
    assert any(len(S.CASES[k]["gs"]) == 2 and len(q["mus"]) == 3 and min(q["mus"]) < 0 for k, q in p.items())
    assert any("limit" in q and len(q["mus"]) == 2 and 0.4 in q["mus"] for q in p.values())
    assert any(q.get("zeta_min", 0.3) >= 1.0 for q in p.values()) and all(q.get("rr_intensity") is None for k, q in
                                                                         ((k, c["params"]) for k, c in S.CASES.items() if k not in RR_CASES))


def test_every_branch_of_the_roulette_is_taken():
    """over the roulette's cases together every branch holds at least 200 rays, and at least 20 inside the cases' longest runs without a
    fragile photon -- where nothing but the float32 bound is allowed (a surface event is small only with zetaMin >= 1, large otherwise:
    `each stage it can take`)"""
    whole = {b: sum(model_for(k).branches[b] for k in RR_CASES) for b in S.BRANCHES}
    clean = {b: sum(clean_model(k).branches[b] for k in RR_CASES) for b in S.BRANCHES}
    assert min(whole.values()) >= 200, whole
    assert min(clean.values()) >= 20, clean
    # (the rays the model skips are the ones it counts as lost, and a flux case or a case without the roulette skips none)
    assert all(model_for(k).counters["raysSkipped"] == model_for(k).branches["small lost"] > 0 for k in RR_CASES)
    assert all(model_for(k).counters["raysSkipped"] == 0 for k in S.CASES if k not in RR_CASES)


def test_tracer_calls_without_the_roulette_are_the_photons_traces_and_one_per_ray():
    for name in ("a common", "h three"):
        c = model_for(name).counters
        nd = len(S.CASES[name]["params"].get("mus", ()))
        rays = nd * (c["scatterings"] + c["surfaceHits"])   # (every event makes its rays: the albedo is above 0)
        assert c["tracerCalls"] == c["scatterings"] + c["surfaceHits"] + c["exitsTop"] + rays


# (variant, case, is it seen on the WHOLE case too?)  On a whole case a fragile photon may carry up to the largest contribution there is
# per ray into any entry, and the counters may differ by the fragile photons' own counts.  A control that only RE-DRAWS the rays' deviates
# -- the fourth counter word d instead of d + 1, a key without the batch: the same distribution from other blocks -- changes the counters
# by a fluctuation of some sqrt(rays), which at 10^4 photons is about what the fragile photons' own counts allow (measured: `r wide` missed
# the word d by 64 skipped rays against 80 allowed; the key without the batch 14178 against 14097, 46813 against 46783 skipped rays, inside
# the allowance), and the tally entries by about a THOUSANDTH of the whole case's tolerance (measured: 0.001 to 0.002 of it; `r wide`
# 0.3 to 0.37): a whole case cannot see a re-draw.  The run without fragile photons, where the float32 bound alone is allowed, sees every
# one of them, on every case -- the device runs that range of every case, and a fused launch, which always starts at photon 0, runs
# S.FUSED_CLEAN_N photons a batch of a key for which the three batches hold no fragile photon (below).  The other controls change WHAT is
# computed and are seen on the whole case `r wide` as well, whose wide columns and contribution limit leave the fragile photons little
# to carry; a downward direction that counts is seen on every whole case (those entries are exactly 0).
RAY_CONTROLS = [("ray block ignores the direction", "r wide", True), ("ray block ignores the direction", "r three", False),
                ("ray block ignores the direction", "r three two components", False),
                ("ray counter word d", "r one up", False), ("ray counter word d", "r three", False), ("ray counter word d", "r wide", False),
                ("r2 from word 0", "r wide", True), ("r2 from word 0", "r zeta", True), ("r2 from word 0", "r one up", False),
                ("second leg from the event", "r wide", True), ("second leg from the event", "r one up", False),
                ("second leg from the event", "r limit", False), ("second leg from the event", "r three two components", False),
                ("downward direction counts", "r one down", True), ("downward direction counts", "r three", True),
                ("downward direction counts", "r three two components", True), ("downward direction counts", "r zeta", True),
                ("downward direction counts", "r wide", True)]


@pytest.mark.parametrize("variant,name,whole", RAY_CONTROLS)
def test_a_mistake_in_the_rays_roulette_fails_the_comparison(variant, name, whole):
    """a ray block that ignores the direction number, or has d instead of d + 1 in its fourth counter word (direction 0: the event's own
    block), r2 from the free path's word, a second leg restarted at the event, a downward direction that counts: each fails the
    comparison the GPU module makes on the case's run without fragile photons, and on the whole case where RAY_CONTROLS says so"""
    base = model_for(name)
    assert S.compare(base, base.tallies, base.counters)[0] == []
    assert _fails(clean_model(name), clean_model(name, variant)), (name, variant)
    if whole:
        assert _fails(base, model_for(name, variant=variant)), (name, variant)


@pytest.mark.parametrize("name", ["r one up", "r three", "r wide"])
def test_a_ray_key_without_the_batch_fails_the_comparison(name):
    """fused launches: batch b's rays keyed as batch 0's (every batch would reuse the same ray deviates).  A re-draw: seen on the run
    without fragile photons (see RAY_CONTROLS)"""
    variant = "ray key without the batch"
    for b in (1, 2):
        base = model_for(name, batch=b)
        assert base.counters == model_for(name, seed=(S.SEED[0], S.SEED[1] + b)).counters   # (batch b of a fused launch: the key's second word + b)
        first, count = S.clean_range(base)
        assert count >= 500
        assert _fails(model_for(name, first=first, n=count, batch=b), model_for(name, first=first, n=count, variant=variant, batch=b)), (name, b)
    assert not _fails(model_for(name), model_for(name, variant=variant))   # (batch 0: nothing to tell apart)


@pytest.mark.parametrize("name", S.FUSED_CLEAN_CASES)
def test_fused_batches_without_a_fragile_photon_see_the_ray_key(name):
    """what the GPU module's fused launch without fragile photons compares: batches 0, 1, 2 of S.FUSED_CLEAN_SEED, photons from 0, none of
    them fragile -- and on exactly those runs a ray key without the batch (a ring record whose batch word is lost does the same) fails"""
    for b in range(3):
        base = model_for(name, seed=S.FUSED_CLEAN_SEED, n=S.FUSED_CLEAN_N, batch=b)
        assert not base.per_photon["fragile"].any(), (name, b, np.nonzero(base.per_photon["fragile"])[0])
        assert min(base.branches[k] for k in ("small lost", "small won counted", "large first leg", "second leg counted")) >= 20, base.branches
        alone = model_for(name, seed=(S.FUSED_CLEAN_SEED[0], S.FUSED_CLEAN_SEED[1] + b), n=S.FUSED_CLEAN_N)
        assert base.counters == alone.counters and all(np.array_equal(base.tallies[k], alone.tallies[k]) for k in base.tallies)
        other = model_for(name, seed=S.FUSED_CLEAN_SEED, n=S.FUSED_CLEAN_N, batch=b, variant="ray key without the batch")
        assert _fails(base, other) == (b > 0), (name, b)
        if b > 0:   # (... by the tallies alone, which is what the device is held to per batch: its ray counters go over the group)
            assert S.compare(base, other.tallies, other.counters, S.COUNTERS_EXACT)[0] != [], (name, b)


def beyond_two_to_the_32(name, first, n=1500):
    """(first photon, count) of the longest run without a fragile photon among the photons of first .. first + n - 1 whose number has a
    high word"""
    base = model_for(name, first=first, n=n)
    at, count = S.clean_range(base, start=max(0, 2 ** 32 - first))
    return first + at, count


@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["r one up", "r three"])
def test_a_ray_block_without_the_high_word_fails_the_comparison(name, first):
    """the ray's block alone keyed without the photon number's high word (the ring record's word, make_ray's second argument): a re-draw of
    the rays' deviates, seen on the run without fragile photons beyond 2^32 that the GPU module launches"""
    at, count = beyond_two_to_the_32(name, first)
    assert at >= 2 ** 32 and count >= 150, (at, count)   # (some hundreds of rays of every kind)
    clean = model_for(name, first=at, n=count)
    assert not clean.per_photon["fragile"].any()
    assert _fails(clean, model_for(name, first=at, n=count, variant="ray block without the high word")), (name, first)


# ---- the diagnostic tallies: level fluxes, track lengths, path moments, the path histogram ----------------------------------------------
DIAGNOSTICS = [(name, kind) for kind in S.KINDS for name in S.DIAGNOSTIC_CASES]
LEAST = 64   # the shortest run of photons the GPU module launches on its own


@pytest.mark.parametrize("name,kind", DIAGNOSTICS + [("a common", "bins")])
def test_fragile_share_of_the_diagnostic_cases(name, kind):
    """a condition on the inputs: with the kind's own decisions (start column, level column, bin) the share stays within the project's
    cap, and the runs without a fragile photon that the GPU module launches hold nine photons in ten"""
    r = diagnostic_model(name, kind)
    assert r.fragile_share <= S.FRAGILE_CAP, (name, kind, r.fragile_share, r.per_photon["why"])
    assert abs(r.fragile_share - S.DIAGNOSTIC_SHARES[kind][name]) < 1e-9, (name, kind, r.fragile_share)   # (the shares written down are the ones measured)
    new = {"levels": ("start column", "level column"), "bins": ("bin",)}.get(kind, ())
    assert all(k in r.per_photon["why"] for k in new[-1:]), r.per_photon["why"]                            # (the new decisions do decide)
    clean = diagnostic_clean(name, kind, least=LEAST)
    assert clean.n >= 0.9 * r.n and not clean.per_photon["fragile"].any(), (name, kind, clean.n)
    assert min(clean.counters[k] for k in ("scatterings", "surfaceHits", "exitsTop")) >= 1000, clean.counters
    assert S.compare(clean, clean.tallies, clean.counters)[0] == []


@pytest.mark.parametrize("kind", S.KINDS)
def test_the_window_across_two_to_the_32_has_runs_on_both_sides(kind):
    """1500 photons of `a absorbing` from 2^32 - 700: what the GPU module launches there are the runs of at least 64 photons without a
    fragile one, and they hold some hundreds of photons below and beyond 2^32.  (The cap on the share is a statement about a case's
    20 000 photons, asserted above; of 1500 photons it allows 7, and the level columns of this window happen to take 9.)"""
    runs = diagnostic_runs("a absorbing", kind, first=2 ** 32 - 700, n=1500, least=LEAST)
    assert sum(c for a, c in runs if a + c <= 2 ** 32) >= 300 and sum(a + c - max(a, 2 ** 32) for a, c in runs if a + c > 2 ** 32) >= 300, runs


def test_clean_runs_are_all_the_maximal_runs():
    r = model_for("a absorbing")
    runs = S.clean_runs(r)
    frag = r.per_photon["fragile"]
    covered = np.zeros(r.n, bool)
    for a, c in runs:
        assert c >= 1 and not frag[a:a + c].any() and (a == 0 or frag[a - 1]) and (a + c == r.n or frag[a + c])
        covered[a:a + c] = True
    assert np.array_equal(covered, ~frag)
    assert max(runs, key=lambda t: t[1]) == S.clean_range(r)
    assert S.clean_runs(r, least=LEAST) == [t for t in runs if t[1] >= LEAST]
    ids = S.run_ids(runs[:3])
    assert len(ids) == sum(c for _, c in runs[:3]) and ids[0] == runs[0][0]
    # ... and the model over those photon numbers is the sum of the model over each run (photons do not know of each other)
    whole = S.run(case_problem("a absorbing"), S.SEED, 0, 0, ids=ids)
    parts = [S.run(case_problem("a absorbing"), S.SEED, a, c) for a, c in runs[:3]]
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    assert all(np.allclose(whole.tallies[k], sum(p.tallies[k] for p in parts), rtol=1e-13, atol=0) for k in whole.tallies)


def _close(a, b, rtol=1e-12):
    return np.allclose(a, b, rtol=rtol, atol=rtol * max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("name", S.DIAGNOSTIC_CASES)
def test_identities_of_the_diagnostic_tallies(name):
    """exact in the model's float64, per column and per photon"""
    import dataclasses

    lev, trk, bins = (diagnostic_model(name, k) for k in ("levels", "tracks", "bins"))
    nz = lev.tallies["levelFluxUp"].shape[0] - 1
    up, down = (lev.caps[k] - 1.0 for k in ("fluxUp", "fluxDown"))            # (a cap is 1 + the photon's own deposit)
    assert _close(lev.tallies["levelFluxDown"][0], lev.tallies["fluxDown"]) and _close(lev.tallies["levelFluxUp"][nz], lev.tallies["fluxUp"])
    assert _close(lev.extras["perPhoton"]["levelFluxDown"][:, 0], down) and _close(lev.extras["perPhoton"]["levelFluxUp"][:, nz], up)
    assert lev.tallies["levelFluxDown"][nz].sum() == lev.n and (lev.extras["perPhoton"]["levelFluxDown"][:, nz] >= 1.0).all()
    # the bins add up to the fluxes, per photon too; the path bins to the first moments of the same problem's path sums
    pp = bins.extras["perPhoton"]
    assert _close(pp["binUp"], bins.caps["fluxUp"] - 1.0) and _close(pp["binDown"], bins.caps["fluxDown"] - 1.0)
    assert _close(bins.tallies["binUp"].sum(), bins.tallies["fluxUp"].sum()) and _close(bins.tallies["binDown"].sum(), bins.tallies["fluxDown"].sum())
    paths = S.run(dataclasses.replace(diagnostic_problem(name, "bins"), extra="paths", bin_edges=None), S.SEED, 0, bins.n)
    assert _close(bins.tallies["binPathUp"].sum(), paths.tallies["pathUp1"].sum()) and _close(bins.tallies["binPathDown"].sum(), paths.tallies["pathDown1"].sum())
    assert _close(pp["binPathUp"], paths.extras["perPhoton"]["pathUp1"]) and _close(pp["binPathDown"], paths.extras["perPhoton"]["pathDown1"])
    assert (paths.tallies["pathUp2"] * paths.tallies["fluxUp"] >= paths.tallies["pathUp1"] ** 2 * (1 - 1e-12)).all()   # (Cauchy-Schwarz, per column)
    # the track lengths of all cells are the photons' weighted segments
    assert _close(trk.extras["perPhoton"]["tracks"], trk.extras["perPhoton"]["wS"])
    assert _close(trk.tallies["tracks"].sum(), trk.extras["perPhoton"]["wS"].sum()) and _close(trk.tallies["tracks"].sum(axis=(1, 2)), trk.tallies["trackLayers"])
    assert (trk.bounds["trackLayers"] <= trk.bounds["tracks"].sum(axis=(1, 2)) * (1 + 1e-12)).all()     # (the transfer terms vanish in a layer's sum)


def test_net_level_flux_is_the_absorption_without_roulette():
    """`f no roulette`: what flows into a layer and not out of it is what the photon leaves there as absorption, photon by photon"""
    r = diagnostic_model("f no roulette", "levels")
    pp = r.extras["perPhoton"]
    net = pp["levelFluxDown"] - pp["levelFluxUp"]
    into = net[:, 1:] - net[:, :-1]
    assert np.abs(into - pp["absLayer"]).max() < 1e-12, np.abs(into - pp["absLayer"]).max()
    assert pp["absLayer"].sum() > 0.3 * r.n


# ... against independent references: batches of the model as above, 4 standard errors of its own batches + SOLVER
DIAGNOSTIC_SLABS = [(1.0, 0.9, 0.5), (1.0, 1.0, 0.0), (10.0, 0.9, 0.5), (10.0, 1.0, 0.0)]


@functools.lru_cache(maxsize=None)
def _slab_batches(tau, omega, albedo, kind):
    import dataclasses
    from tests.test_plane_parallel import MOMENTS

    n, nb = (30_000 if tau < 5 else 10_000), 10
    P = dataclasses.replace(_slab(tau, omega, albedo, MOMENTS), extra=kind)
    return P, [S.run(P, (10, b), 0, n) for b in range(1, nb + 1)]


def _mean_se(per):
    per = np.asarray(per)
    return per.mean(0), per.std(0, ddof=1) / np.sqrt(len(per))


@pytest.mark.parametrize("tau,omega,albedo", DIAGNOSTIC_SLABS)
def test_model_level_fluxes_against_the_level_solver(tau, omega, albedo):
    from tests.level_flux_solver import solve_levels
    from tests.test_plane_parallel import G, MU0, _sampled_moments

    P, rs = _slab_batches(tau, omega, albedo, "levels")
    ze = P.ze.astype(np.float64)
    depth = tau * (ze[-1] - ze) / (ze[-1] - ze[0])                      # optical depth above level k
    want = solve_levels(depth, tau, omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    for key, ref in zip(("levelFluxUp", "levelFluxDown"), want):
        got, se = _mean_se([r.tallies[key].sum(axis=(1, 2)) / r.n for r in rs])
        assert (np.abs(got - ref) <= 4.0 * se + SOLVER).all(), (key, tau, omega, albedo, got - ref, se)


@pytest.mark.parametrize("tau,omega,albedo", DIAGNOSTIC_SLABS)
def test_model_mean_paths_against_the_equivalence_theorem(tau, omega, albedo):
    """<L> of the reflected and of the transmitted light, and <L^2>, against the figures tests/test_gpu_path_lengths.py derives from the
    adding-doubling solver; the reference's own finite-difference uncertainty is added as it is there"""
    from tests.test_gpu_path_lengths import _solver_moments

    P, rs = _slab_batches(tau, omega, albedo, "paths")
    H = float(P.ze[-1]) - float(P.ze[0])
    per = [[r.tallies["pathUp1"].sum() / r.tallies["fluxUp"].sum() / H, r.tallies["pathDown1"].sum() / r.tallies["fluxDown"].sum() / H,
            r.tallies["pathUp2"].sum() / r.tallies["fluxUp"].sum() / H ** 2, r.tallies["pathDown2"].sum() / r.tallies["fluxDown"].sum() / H ** 2] for r in rs]
    got, se = _mean_se(per)
    m1, m2, u1, u2 = _solver_moments(tau, omega, albedo)
    want, unc = np.concatenate([m1, m2]), np.concatenate([u1, u2])
    assert (want[:2] > 0.5).all() and (se > 0).all()
    assert (np.abs(got - want) <= 4.0 * se + SOLVER + unc).all(), (tau, omega, albedo, got - want, se, unc)


@pytest.mark.parametrize("tau,albedo", [(1.0, 0.0), (1.0, 0.5), (10.0, 0.0), (10.0, 0.5)])
def test_model_actinic_flux_against_the_net_flux_divergence(tau, albedo):
    """(1 - omega) sigma dz <actinic flux> of a layer is what the layer absorbs: the solver's net flux into it less the net flux out"""
    from tests.level_flux_solver import solve_levels
    from tests.test_plane_parallel import G, MU0, _sampled_moments

    omega = 0.9
    P, rs = _slab_batches(tau, omega, albedo, "tracks")
    ze = P.ze.astype(np.float64)
    sigma, om = float(P.ext[0, 0]), float(P.ssa[0, 0])
    depth = sigma * (ze[-1] - ze)
    up, down = solve_levels(depth, depth[0], omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    net = down - up
    want = net[1:] - net[:-1]
    got, se = _mean_se([(1.0 - om) * sigma * r.tallies["trackLayers"] / r.n for r in rs])
    assert (want > 1e-3).all()
    assert (np.abs(got - want) <= 4.0 * se + SOLVER).all(), (tau, albedo, got - want, se)
    # ... and it is the model's own absorption, batch by batch, within the sampling of the collisions
    own, se_own = _mean_se([(1.0 - om) * sigma * r.tallies["trackLayers"] / r.n - r.tallies["volumeAbsorption"].sum(axis=(1, 2)) / r.n for r in rs])
    assert (np.abs(own) <= 4.0 * se_own + SOLVER).all(), (own, se_own)


# ... the conditions on the inputs
@pytest.mark.parametrize("name", S.DIAGNOSTIC_CASES + ("a common",))
def test_the_histograms_edges_suit_the_case(name):
    e = S.bin_edges(name).astype(np.float64)
    first, ratio, nbins = S.BIN_EDGES[name]
    assert e.dtype == np.float64 and len(e) == nbins + 1 and e[0] == 0 and np.allclose(e[2:] / e[1:-1], ratio, rtol=1e-6)   # a geometric progression behind 0
    r = diagnostic_model(name, "bins")
    D = r.extras["deposits"]
    b = np.clip(np.searchsorted(e, D[1].astype(np.float32).astype(np.float64), side="right") - 1, 0, nbins)
    count = np.bincount(b, minlength=nbins + 1)
    weight = r.tallies["binUp"] + r.tallies["binDown"]
    assert np.allclose(np.bincount(b, weights=D[3], minlength=nbins + 1), weight, rtol=1e-12)
    assert count[-1] > 0 and 0 < weight[-1] < 0.01 * weight.sum(), (name, count[-1], weight[-1] / weight.sum())
    assert (count[:-1] >= 100).sum() >= 20, (name, count)
    direct = S.unscattered_path(diagnostic_problem(name, "bins"))
    assert np.abs(e[1:] / direct - 1.0).min() > 1e-4, (name, direct)     # (else every direct-beam photon would be fragile at once)
    # (... the direct beam's share of the case, exp(-tau / mu0) of its photons within five binomial standard deviations)
    P = diagnostic_problem(name, "bins")
    share = float(np.exp(-np.sum(P.ext.astype(np.float64).sum(0) * np.diff(P.ze.astype(np.float64))) / abs(float(S.direction(-abs(P.mu0), P.azimuth)[2]))))
    unscattered = np.count_nonzero((np.abs(D[1] / direct - 1.0) < 1e-12) & (D[4] == 0))
    assert abs(unscattered - share * r.n) <= 5.0 * np.sqrt(share * (1.0 - share) * r.n), (name, unscattered, share * r.n)


@pytest.mark.parametrize("name", S.DIAGNOSTIC_CASES)
def test_the_track_bounds_resolve_what_the_statistics_do_not(name):
    """in every cell that receives 1000 pieces the summed bound is at most 1e-3 of the entry (a wider bound would pin nothing the
    statistical tests do not pin already), on the whole case and over the photons the GPU module launches"""
    for r in (diagnostic_model(name, "tracks"), diagnostic_clean(name, "tracks", least=LEAST)):
        big = r.extras["trackPieces"] >= S.TRACK_PIECES
        assert big.sum() >= 0.9 * big.size, (name, big.sum())
        worst = float((r.bounds["tracks"][big] / r.tallies["tracks"][big]).max())
        assert worst <= S.TRACK_RESOLUTION, (name, worst)
        assert (r.bounds["trackLayers"] / r.tallies["trackLayers"]).max() <= 0.3 * S.TRACK_RESOLUTION


# ... the controls: a model with one changed convention must FAIL the comparison the GPU module makes -- over the photons that are not
# fragile, with the float32 bound alone -- on every case listed (a black surface reflects nothing and a white one keeps the weight:
# `g black` cannot see the reflection's controls, `g white` not the weight after it)
DIAGNOSTIC_CONTROLS = [(kind, variant, name) for kind in S.KINDS for variant in S.EXTRA_VARIANTS[kind] for name in ("a absorbing", "c two")]


@pytest.mark.parametrize("kind,variant,name", DIAGNOSTIC_CONTROLS)
def test_a_changed_convention_of_a_diagnostic_tally_fails_the_comparison(kind, variant, name):
    base = diagnostic_clean(name, kind, least=LEAST)
    other = diagnostic_clean(name, kind, variant=variant, least=LEAST)
    assert base.counters == other.counters                       # (the photons are the same: only the bookkeeping differs)
    miss, _ = S.compare(base, other.tallies, other.counters)
    fields = {m[0] for m in miss}
    assert fields and fields <= set(S.EXTRA_FIELDS[kind] + S.DERIVED_FIELDS), (kind, variant, name, fields)


def test_the_controls_are_the_eleven_asked_for():
    assert len({v for vs in S.EXTRA_VARIANTS.values() for v in vs}) == 11
    assert set(S.EXTRA_VARIANTS["paths"]) < set(S.EXTRA_VARIANTS["bins"]) and len(S.EXTRA_VARIANTS["levels"]) == 4 and len(S.EXTRA_VARIANTS["tracks"]) == 3
