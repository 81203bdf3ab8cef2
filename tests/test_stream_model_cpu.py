"""The float64 stream model (tests/stream_model.py) is right on its own, and its tolerances would catch a subtly wrong kernel --
both shown without a GPU:

  * Philox known answers (Random123's kat_vectors for philox4x32-10) for tests/philox_ref.py and the model's vectorised form;
  * the model against the adding-doubling solver on the cases of tests/test_plane_parallel.py, 4 standard errors of its own sample;
  * the model against the CPU oracle on a two-component layered case with a reflecting surface and a radiance direction
    (two independent samples: combined standard errors);
  * the share of fragile photons of every shared case, asserted below 0.5 % (a condition on the inputs);
  * energy: up + absorbed + (1 - albedo) down = 1 per photon without roulette;
  * the controls: a model that swaps first() and second(), takes the azimuth from first(), interpolates the inverse table one
    interval on, or drops the high word of the photon number must FAIL the comparison the GPU module makes, at the shared cases' sizes.
    (The fourth control the issue names -- a ray block that ignores the direction number -- has nothing to act on: that block is drawn
    only by the local estimate's own roulette, which the model leaves to the replay and oracle tests.)"""
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
def model_for(name, seed=S.SEED, first=0, n=None, variant=None, drop=False):
    return S.run(case_problem(name), seed, first, n or S.CASES[name]["n"], variant=variant, drop_high_word=drop)


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
def _slab(tau, omega, albedo, moments, dirs=None, n_table=10001):
    from tools import cases

    d = cases.plane_parallel(optical_depth=tau, ssa=omega, nx=2, ny=2, nlayers=3)
    t = M.PhaseFunctionTable([M.henyey_greenstein(0.85, moments)])
    fwd = [t.forward_table(n_table)] if dirs is not None else None
    return S.Problem(d["xe"], d["ye"], d["ze"], d["ext"][:, 0, 0], d["ssa"][:, 0, 0], d["pf"][:, 0, 0], [t.inverse_table(n_table)],
                     mu0=0.5, azimuth=0.0, albedo=albedo, roulette=True, dirs=dirs, fwd=fwd)


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


@pytest.mark.parametrize("tau,omega,albedo", [(1.0, 1.0, 0.0), (10.0, 0.9, 0.5), (0.1, 1.0, 0.5)])
def test_model_radiances_against_adding_doubling(tau, omega, albedo):
    from tests.plane_parallel_solver import solve
    from tests.test_plane_parallel import G, MOMENTS_RADIANCE, MU0, VIEW_MUS, VIEW_PHIS

    n, nb = (60_000 if tau < 5 else 20_000), 10
    dirs = np.array([S.direction(m, p) for m, p in zip(VIEW_MUS, VIEW_PHIS)])
    P = _slab(tau, omega, albedo, MOMENTS_RADIANCE, dirs)
    rs = [S.run(P, (10, b), 0, n) for b in range(1, nb + 1)]
    want = solve(tau, omega, G, MU0, albedo=albedo, radiance_mus=VIEW_MUS, radiance_dphis_deg=VIEW_PHIS)
    per = np.array([r.tallies["intensity"].sum(axis=(0, 2, 3)) / r.n for r in rs])   # (mean over columns of sum / photons per column)
    got, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(nb)
    for k in range(len(VIEW_MUS)):
        assert abs(got[k] - want["intensity"][k]) <= 4.0 * se[k] + SOLVER, (k, tau, omega, albedo, got[k], want["intensity"][k], se[k])


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


# ---- the inputs: few fragile photons --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_fragile_share_of_the_shared_cases(name):
    r = model_for(name)
    assert r.fragile_share <= S.FRAGILE_CAP, (name, r.fragile_share, r.per_photon["why"])
    assert r.counters["scatterings"] > 0 and r.counters["surfaceHits"] > 0 and r.counters["exitsTop"] > 0
    assert abs(r.fragile_share - S.FRAGILE_SHARES[name]) < 1e-9, (name, r.fragile_share)   # (the shares written down are the ones measured)


@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["a common", "h three"])
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


@pytest.mark.parametrize("name", ["a common", "h three"])
@pytest.mark.parametrize("first", [2 ** 32 - 700, 2 ** 33 + 5])
def test_a_dropped_high_word_fails_the_comparison(name, first):
    base = model_for(name, first=first, n=1500)
    assert _fails(base, model_for(name, first=first, n=1500, drop=True)), (name, first)
