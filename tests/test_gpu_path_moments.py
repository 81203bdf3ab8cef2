"""Batch statistics of the two path tallies on the device (i3rc_hip_run_batches_path_moments, through the mirror's
computeRadiativeTransferPathMoments): the path-length fields, their column means and the domain's <L>, <L^2> -- or the path histogram
and the two bounds of R(k) at the coefficients of i3rc_hip_set_path_spectrum -- of a loop's batches, normalised and added up, x and
x^2, by moments_fields_kernel<PathFields> / path_quantities_kernel behind every batch's launch.

  the loop is its batches   s1, s2 against the same batches run one by one (computeRadiativeTransfer + reportResults; the domain ratios
                            and the spectrum restated on the host from every batch's raw block, tests/path_moments.py), ordinary moments
                            and counters included, once per place of the extinction field and kind; the histogram with its sums in LDS
                            and in global memory
  one batch, bit for bit    where a batch's sums do not depend on their order: s1 = float64(field), s2 = s1 s1
  identities                <L> x meanFluxUp = meanPathLengthUp batch by batch; the spectrum at k = 0 is the mean flux; lower <= upper
  statistics                mean and standard error of <L>, <L^2> and of the spectrum against the adding-doubling solver
  launches                  more batches than slots, batches below a wavefront, split batches, a second call, the refusals

Tolerances: those of tests/test_gpu_diagnostic_moments.py.  The device adds the float32 values the host reports, in float64: 1e-9 on
the sums of the fields, 2e-9 on those of their squares; the means, the domain ratios and the spectrum are a tree sum on the device
against the host's: 2e-6 and 4e-6.  A spectrum word holds the device's exp against numpy's, both within an ulp of float64, so that the
one rounding to float32 may fall to the neighbour: one float32 ulp per batch more.  Split batches: tests/sums.py, plus one float32
rounding of every batch's value."""
import ctypes as C

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests import path_moments as P
from tests.extra_tally import PLACES, run, step_cloud_3d
from tests.sums import F32_ULP, order_rtol
from tests.test_gpu_diagnostic_moments import N, NB, SEED
from tests.test_gpu_parity import hg_table, make_gpu

pytestmark = pytest.mark.gpu

B = M.binding
f32 = np.float32
PATH_NAMES, BIN_NAMES = M.host.PATH_LENGTH_NAMES, M.host.PATH_HISTOGRAM_NAMES
BIN_WORD = B.PLAN_BIN_NAME
WHO = "i3rc_hip_run_batches_path_moments"
assert (NB, N) == (5, 3001)
# seven edges in units of the domain's depth: the step cloud's reflected light reaches every bin, the overflow bin included
SEVEN_EDGES = np.array([0.0, 0.4, 1.0, 1.6, 2.4, 3.3, 4.5])
KINDS = {"paths": dict(stream="PhiloxPathStream", fields=PATH_NAMES, scalars=P.SCALARS),
         "bins": dict(stream="PhiloxBinStream", fields=BIN_NAMES, scalars=P.SPECTRUM)}


def _switch(kind, depth):
    """the parameters that switch the kind on, over a domain of this depth: k = (0, 0.5 / H, 5 / H)"""
    if kind == "paths":
        return dict(computePathLengths=True)
    return dict(pathHistogramEdges=f32(SEVEN_EDGES * depth), absorptionCoefficients=f32(np.array([0.0, 0.5, 5.0]) / depth))


def _depth(d):
    return float(d["ze"][-1] - d["ze"][0])


def _raw_fields(g, res, kind):
    """the kind's four raw fields of a batch, and the raw fluxUp, fluxDown"""
    lay, ncol = g.layout(), g.nx * g.ny
    first = lay.counters + B.NUM_COUNTERS
    n = ncol if kind == "paths" else g.pathHistogramEdges.size
    assert len(res["raw"]) == first + 4 * n
    return [res["raw"][first + f * n:first + (f + 1) * n] for f in range(4)], res["raw"][lay.fluxUp:lay.fluxUp + ncol], res["raw"][lay.fluxDown:lay.fluxDown + ncol]


def one_by_one(g, kind, nb, n, seed=SEED, sun=K.SOURCE):
    """the loop's batches through computeRadiativeTransfer + reportResults: per-batch dicts of everything the moments hold -- the column
    means (the plain mean, rounded once), the domain ratios and the spectrum formed here from the batch's raw block --, and the counters
    summed"""
    per, counters = [], None
    for b in range(nb):
        res = run(g, n, seed=(seed[0], seed[1] + b), sun=sun)
        rep = dict(g.reportResults(**{k: True for k in KINDS[kind]["fields"]}))
        fields, up, down = _raw_fields(g, res, kind)
        if kind == "paths":
            for name, field in zip(P.SCALARS[:4], PATH_NAMES):
                rep[name] = np.float32(np.asarray(rep[field], np.float64).mean())
            rep.update(zip(P.SCALARS[4:], P.domain_ratios(fields, up, down)))
        else:
            ks, photons = g.absorptionCoefficients, res["counters"]["photons"]
            for d in range(2):
                lower, upper = P.spectrum_bounds(fields[2 * d], fields[2 * d + 1], g.pathHistogramEdges, ks, photons)
                rep[P.SPECTRUM[2 * d]], rep[P.SPECTRUM[2 * d + 1]] = np.float32(lower), np.float32(upper)
        per.append(rep)
        counters = dict(res["counters"]) if counters is None else {k: counters[k] + v for k, v in res["counters"].items()}
    return per, counters


def _tolerance(key):
    if key.startswith("spectrum"):
        return 2e-6 + F32_ULP
    return 2e-6 if key.startswith(("mean", "domain")) or key == "absorbedProfile" else 1e-9


def assert_moments_are_the_batches(s1, s2, per, what):
    assert set(KINDS[what[0]]["fields"] + KINDS[what[0]]["scalars"]) <= set(s1) and set(s1) == set(s2) == set(per[0]), (sorted(s1), sorted(per[0]))
    for key in s1:
        x = np.stack([np.asarray(p[key], np.float64) for p in per])
        want1, want2 = x.sum(0), (x * x).sum(0)
        tol = _tolerance(key)
        print(what, key, "largest relative difference", float((np.abs(s1[key] - want1) / np.maximum(np.abs(want1), 1e-300)).max()), "allowed", tol)
        assert np.shape(s1[key]) == want1.shape, (what, key, np.shape(s1[key]), want1.shape)
        assert np.allclose(s1[key], want1, rtol=tol, atol=1e-12), (what, key, np.abs(s1[key] - want1).max())
        assert np.allclose(s2[key], want2, rtol=2 * tol, atol=1e-12), (what, key, np.abs(s2[key] - want2).max())


# ---- 1: the loop is its batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place,domain", PLACES, ids=[p for p, _ in PLACES])
@pytest.mark.parametrize("case", ["paths", "bins in LDS", "bins in global memory"])
def test_the_loop_is_its_batches(case, place, domain):
    """step_cloud_3d(0.9) wherever its field can lie; records over a base profile need a second component: that place has the recipe's
    own domain (tests/extra_tally.py, PLACES)"""
    kind = case.split()[0]
    if place == "GRID_COLBASE":
        d, tabs = K.DOMAINS[domain]()
    else:
        d, tabs = step_cloud_3d(0.9), hg_table()
    g = make_gpu(d, tabs, surfaceAlbedo=0.3, **_switch(kind, _depth(d)))
    g.select_grid_place(K.PLACE_KNOB[place])
    if case == "bins in global memory":
        g.set_lds_tallies(False)
    s1, s2, cnt = g.computeRadiativeTransferPathMoments(SEED, NB, *K.SOURCE, N)
    assert g.kernel_name() == f"photon_kernel<{KINDS[kind]['stream']}, false, true, {place}>", g.kernel_name()
    if kind == "bins":
        assert g.last_plan()[BIN_WORD] == int(case == "bins in LDS"), g.last_plan()
    per, counters = one_by_one(g, kind, NB, N)
    assert g.kernel_name() == f"photon_kernel<{KINDS[kind]['stream']}, false, true, {place}>", g.kernel_name()
    assert cnt == counters and cnt["photons"] == NB * N and cnt["scatterings"] > 0, (cnt, counters)
    assert_moments_are_the_batches(s1, s2, per, (kind, place))
    if kind == "bins":      # light in every bin, the overflow bin included; an absorber that matters
        assert np.count_nonzero(s1["pathHistogramUp"]) >= 4 and np.count_nonzero(s1["pathHistogramDown"]) >= 3, (s1["pathHistogramUp"], s1["pathHistogramDown"])
        assert place == "GRID_COLBASE" or s1["pathHistogramUp"][-1] > 0, s1["pathHistogramUp"]      # (the step cloud: reflected light beyond 4.5 depths)
        assert 0 < s1["spectrumUpLower"][2] < s1["spectrumUpUpper"][2] < s1["spectrumUpUpper"][0]
    else:
        assert s1["domainPathUp"] > 0 and s1["domainPathDown"] > NB * _depth(d)      # (no path through the domain is shorter than its depth)
    g.finalize_Integrator()


# ---- 2: one batch, bit for bit -----------------------------------------------------------------------------------------------------------
def _unequal_x(d):
    nx = len(d["xe"]) - 1
    xe = np.cumsum(np.concatenate([[0.0], 0.04 + 0.015 * (np.arange(nx) % 3)])).astype(np.float32)
    assert np.ptp(np.diff(xe)) > 0.01
    return dict(d, xe=xe)


@pytest.mark.parametrize("case", ["paths, regular", "paths, irregular", "bins"])
def test_one_batch_bit_for_bit(case):
    """The clear 8 x 4 x 6 domain under a zenith sun over a black surface: every photon arrives at the surface with weight 1 and the
    path L0 = 2.5 - 2^-22 (tests/test_gpu_path_lengths.py), 24 significant bits -- a sum of up to 2^29 such terms is exact in float64
    in any order; L0^2 has 47, so a column's sum of squares is exact up to 64 photons, which is why the path lengths run 601 photons
    over the 32 columns (asserted).  Two runs of the batch then give one raw block, and host and kernel round it by one statement."""
    from tests.test_gpu_path_lengths import CLOUD_Z, _clear_domain, _straight_path

    kind = case.split(",")[0]
    d = _clear_domain("8x4x6")
    L0 = _straight_path(CLOUD_Z)
    assert L0 == 2.5 - 2.0 ** -22
    if case == "paths, irregular":
        d = _unequal_x(d)
    n = 601 if kind == "paths" else N
    params = dict(computePathLengths=True) if kind == "paths" else dict(pathHistogramEdges=f32([0.0, 1.0, 2.0, 3.0, 4.0]), absorptionCoefficients=f32([0.0, 0.7, 9.0]))
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, **params)
    s1, s2, cnt = g.computeRadiativeTransferPathMoments(SEED, 1, 1.0, 0.0, n)
    (want,), counters = one_by_one(g, kind, 1, n, sun=(1.0, 0.0))
    assert cnt == counters and cnt["photons"] == n and cnt["dropped"] == 0 and cnt["scatterings"] == 0 and cnt["surfaceHits"] == n, cnt
    if kind == "paths":
        down = g.fetch()[g.layout().fluxDown:][:32]
        assert down.sum() == n and 0 < down.max() <= 64, down
        live, dead = ("pathLengthDown", "pathLengthSquaredDown"), ("pathLengthUp", "pathLengthSquaredUp")
    else:
        assert want["pathHistogramDown"][2] == 1 and np.count_nonzero(want["pathHistogramDown"]) == 1      # all light in one bin
        live, dead = ("pathHistogramDown", "pathHistogramPathDown"), ("pathHistogramUp", "pathHistogramPathUp")
    for key in live + dead:
        w = np.asarray(want[key], np.float64)
        assert (w.max() > 0) == (key in live), key
        assert np.array_equal(s1[key].view(np.uint64), w.view(np.uint64)), (key, np.argwhere(s1[key] != w)[:8])
        assert np.array_equal(s2[key].view(np.uint64), (w * w).view(np.uint64)), key
    if kind == "paths":
        assert len(np.unique(want["pathLengthDown"])) > (1 if case == "paths, regular" else 4)
        # every column's mean path is L0, so the domain's is: the ratio of two exact sums, rounded once
        assert s1["domainPathDown"] == float(f32(L0)) and s2["domainPathDown"] == s1["domainPathDown"] ** 2 and s1["domainPathUp"] == 0 and s1["domainPathSquaredUp"] == 0
        # (the domain's sum of squares has 601 terms and is not exact: the host's ratio, to the rounding that may fall to the neighbour)
        assert abs(s1["domainPathSquaredDown"] - float(want["domainPathSquaredDown"])) <= float(np.spacing(want["domainPathSquaredDown"]))
        assert abs(s1["domainPathSquaredDown"] - L0 * L0) <= F32_ULP * L0 * L0 and s2["domainPathSquaredDown"] == s1["domainPathSquaredDown"] ** 2
    else:
        # one bin holds all the light: a sum of one term, and exp(-k L0) between the bounds
        for key in P.SPECTRUM:
            w = np.asarray(want[key], np.float64)
            assert np.all(np.abs(s1[key] - w) <= np.spacing(f32(w)).astype(np.float64)), (key, s1[key], w)
        assert (s1["spectrumUpLower"] == 0).all() and (s1["spectrumUpUpper"] == 0).all()
        ks = g.absorptionCoefficients.astype(np.float64)
        assert s1["spectrumDownLower"][0] == 1 and s1["spectrumDownUpper"][0] == 1
        assert np.allclose(s1["spectrumDownLower"], np.exp(-ks * L0), rtol=2 * F32_ULP, atol=0)
        assert (s1["spectrumDownLower"][1:] < s1["spectrumDownUpper"][1:]).all() and (s1["spectrumDownUpper"] <= np.exp(-ks * 2.0) * (1 + F32_ULP)).all()
    g.finalize_Integrator()


# ---- 3: identities inside one call -------------------------------------------------------------------------------------------------------
def test_the_domain_path_times_the_mean_flux_is_the_mean_path_length():
    """On a regular grid meanFluxUp is the domain's flux per photon and meanPathLengthUp its path sum per photon, so batch by batch
    domainPathUp x meanFluxUp = meanPathLengthUp to the five float32 roundings involved (two fields, two means, the ratio: 2.5 ulps).
    The batches' own values come from calls of one batch each, whose sums must be the loop's."""
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3, computePathLengths=True)
    s1, s2, cnt = g.computeRadiativeTransferPathMoments(SEED, NB, *K.SOURCE, N)
    singles = [g.computeRadiativeTransferPathMoments((SEED[0], SEED[1] + b), 1, *K.SOURCE, N)[0] for b in range(NB)]
    for key in P.SCALARS + ("meanFluxUp", "meanFluxDown"):
        total = sum(float(s[key]) for s in singles)
        assert abs(total - s1[key]) <= 1e-12 * abs(total), (key, total, s1[key])
        assert abs(sum(float(s[key]) ** 2 for s in singles) - s2[key]) <= 1e-12 * s2[key], key
    for way in ("Up", "Down"):
        for path, mean in (("domainPath" + way, "meanPathLength" + way), ("domainPathSquared" + way, "meanPathLengthSquared" + way)):
            got = sum(float(s[path]) * float(s["meanFlux" + way]) for s in singles)
            print(path, "x meanFlux" + way, got, mean, float(s1[mean]), "difference in float32 ulps", abs(got - s1[mean]) / (F32_ULP * s1[mean]), "allowed", NB)
            assert s1[mean] > 0 and abs(got - s1[mean]) <= NB * F32_ULP * s1[mean], (path, got, s1[mean])
    g.finalize_Integrator()


def test_the_spectrum_without_absorption_is_the_mean_flux():
    d = step_cloud_3d(0.9)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, **_switch("bins", _depth(d)))
    s1, _, cnt = g.computeRadiativeTransferPathMoments(SEED, NB, *K.SOURCE, N)
    for way in ("Up", "Down"):
        lower, upper, flux = s1[f"spectrum{way}Lower"], s1[f"spectrum{way}Upper"], float(s1["meanFlux" + way])
        print(way, "k = 0:", lower[0], upper[0], "meanFlux", flux, "allowed", NB * F32_ULP * flux)
        assert flux > 0 and abs(lower[0] - flux) <= NB * F32_ULP * flux and abs(upper[0] - flux) <= NB * F32_ULP * flux
        assert (lower <= upper).all() and (np.diff(upper) < 0).all() and (np.diff(lower) < 0).all(), (lower, upper)
        # ... and the bins add up to it as well
        assert abs(s1[f"pathHistogram{way}"].sum() - flux) <= NB * F32_ULP * flux
    g.finalize_Integrator()


# ---- 4: the statistics are usable --------------------------------------------------------------------------------------------------------
TAU_A = (0.05, 0.5, 2.0)        # (tests/test_path_moments_cpu.py: no reference ratio of the four slabs is below 1e-3 at these)
SLABS = [(tau, omega, albedo) for tau in (1.0, 10.0) for omega, albedo in ((0.9, 0.5), (1.0, 0.0))]
STAT_NB, STAT_N, H = 20, 100_000, 1.0


def _slab(tau, omega, albedo, **params):
    from tests.test_gpu_path_lengths import SLAB_Z
    from tests.test_plane_parallel import G, MOMENTS

    ext = np.full((4, 1, 1), f32(tau / H), np.float32)
    d = dict(xe=np.array([0.0, 4.0], np.float32), ye=np.array([0.0, 4.0], np.float32), ze=SLAB_Z * f32(H), ext=ext,
             ssa=np.full_like(ext, f32(omega)), pf=np.ones(ext.shape, np.int32))
    return make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, **params)


def _drivers_mean_and_error(s1, s2, nb):
    """as the drivers form them, in real(4): m = s / nb, se = sqrt(max(0, m2 - m1^2) / (nb - 1))"""
    m1, m2 = f32(s1) / f32(nb), f32(s2) / f32(nb)
    return m1, np.sqrt(np.maximum(f32(0), m2 - m1 * m1) / f32(nb - 1))


@pytest.mark.parametrize("tau,omega,albedo", SLABS)
def test_the_domain_paths_and_their_standard_errors_against_the_adding_solver(tau, omega, albedo):
    """the photons of tests/test_gpu_path_lengths.py::test_mean_paths_against_the_adding_solver, their statistics from the device"""
    from tests.test_gpu_path_lengths import _solver_moments
    from tests.test_plane_parallel import MU0, SIGMAS

    g = _slab(tau, omega, albedo, computePathLengths=True)
    s1, s2, cnt = g.computeRadiativeTransferPathMoments((12, 1), STAT_NB, MU0, 0.0, STAT_N)
    assert cnt["photons"] == STAT_NB * STAT_N
    g.finalize_Integrator()
    m1, m2, u1, u2 = _solver_moments(tau, omega, albedo)
    names = ("domainPathUp", "domainPathDown", "domainPathSquaredUp", "domainPathSquaredDown")
    want, unc = np.concatenate([m1, m2]), np.concatenate([u1, u2])
    for k, name in enumerate(names):
        mean, se = _drivers_mean_and_error(s1[name], s2[name], STAT_NB)
        print(f"tau {tau} omega {omega} albedo {albedo} {name}: {mean:.6f} +- {se:.6f}, solver {want[k]:.6f} +- {unc[k]:.2e}, "
              f"difference / tolerance {abs(mean - want[k]) / (SIGMAS * se + unc[k]):.3f}")
        assert se > 0 and unc[k] < 0.25 * se, ("the reference is not sharp enough for this run", name, unc[k], se)
        assert abs(mean - want[k]) <= SIGMAS * se + unc[k], (tau, omega, albedo, name, mean, want[k], se, unc[k])


@pytest.mark.parametrize("tau,omega,albedo", SLABS)
def test_the_spectrum_brackets_the_adding_solver(tau, omega, albedo):
    """the photons of tests/test_gpu_path_histogram.py::test_equivalence_theorem_against_the_adding_solver: for every absorber depth and
    direction the solver's absolute flux of the slab with the absorber mixed in lies between the two bounds, each widened by 4 of its own
    standard errors (the upper one also by what the solver does not model).  Nothing is left out."""
    from tests.plane_parallel_solver import solve
    from tests.test_gpu_path_histogram import THEOREM_EDGES
    from tests.test_plane_parallel import G, MODEL, MU0, SIGMAS, _sampled_moments

    assert SIGMAS == 4 and MODEL == 3e-5
    g = _slab(tau, omega, albedo, pathHistogramEdges=THEOREM_EDGES, absorptionCoefficients=f32(np.array(TAU_A) / H))
    s1, s2, cnt = g.computeRadiativeTransferPathMoments((12, 1), STAT_NB, MU0, 0.0, STAT_N)
    assert cnt["photons"] == STAT_NB * STAT_N and g.last_plan()[BIN_WORD] == 1
    g.finalize_Integrator()
    for j, t in enumerate(TAU_A):
        ref = solve(tau + t, omega * tau / (tau + t), G, MU0, albedo=albedo, chi=_sampled_moments())
        for way in ("Up", "Down"):
            F = ref["flux" + way]
            lo, se_lo = _drivers_mean_and_error(s1[f"spectrum{way}Lower"][j], s2[f"spectrum{way}Lower"][j], STAT_NB)
            hi, se_hi = _drivers_mean_and_error(s1[f"spectrum{way}Upper"][j], s2[f"spectrum{way}Upper"][j], STAT_NB)
            half = 0.5 * (float(hi) - float(lo))
            print(f"tau {tau} omega {omega} albedo {albedo} tau_a {t} flux{way}: [{lo:.6e}, {hi:.6e}] solver {F:.6e}, s.e. {se_lo:.2e} / {se_hi:.2e}, "
                  f"half-width / s.e. {half / min(se_lo, se_hi):.3f}")
            assert 0 < lo <= hi and se_lo > 0 and se_hi > 0
            assert half < 0.25 * min(se_lo, se_hi), ("the edges are not fine enough for this run", t, way, half, se_lo, se_hi)
            assert lo - SIGMAS * se_lo <= F <= hi + SIGMAS * se_hi + MODEL, (tau, omega, albedo, t, way, lo, hi, F, se_lo, se_hi)


# ---- 5: launch mechanics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_more_batches_than_slots_small_batches_and_a_second_call(kind):
    d = step_cloud_3d(0.9)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, **_switch(kind, _depth(d)))
    for nb, n in ((7, N), (7, 1), (3, 63)):        # 7 batches: one more than the slots; a batch of one photon; a batch below a wavefront
        s1, s2, cnt = g.computeRadiativeTransferPathMoments(SEED, nb, *K.SOURCE, n)
        per, counters = one_by_one(g, kind, nb, n)
        assert cnt == counters and cnt["photons"] == nb * n
        assert_moments_are_the_batches(s1, s2, per, (kind, nb, n))
    # (each call above started from zeroed moments: a loop of 7 batches, then shorter ones); and the same call again gives the same sums
    t1, t2, _ = g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 63)
    for key in KINDS[kind]["fields"] + KINDS[kind]["scalars"]:
        assert np.allclose(t1[key], s1[key], rtol=1e-12, atol=0) and np.allclose(t2[key], s2[key], rtol=1e-12, atol=0), key
    g.finalize_Integrator()


@pytest.mark.parametrize("kind", list(KINDS))
def test_split_batches_give_the_unsplit_sums(kind):
    """i3rc_hip_set_launch_limit cuts every batch into launches of 1000 photons: the same increments in another order (tests/sums.py) in
    every raw word, then one float32 rounding per batch that may fall to the neighbour.  A domain ratio has two such sums, a spectrum
    word a sum of bins each of which has two: twice the order bound."""
    d = step_cloud_3d(0.9)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, **_switch(kind, _depth(d)))
    whole1, whole2, cnt = g.computeRadiativeTransferPathMoments(SEED, NB, *K.SOURCE, N)
    launches = g.timed_launches()
    assert B.load().i3rc_hip_set_launch_limit(g._h, 1000) == 0
    part1, part2, cnt2 = g.computeRadiativeTransferPathMoments(SEED, NB, *K.SOURCE, N)
    assert g.timed_launches() - launches == NB * 4 and cnt2 == cnt
    assert B.load().i3rc_hip_set_launch_limit(g._h, 0) == 0
    for key in KINDS[kind]["fields"] + KINDS[kind]["scalars"]:
        rtol = (1 if key in KINDS[kind]["fields"] else 2) * order_rtol(cnt) + F32_ULP
        assert np.all(np.abs(part1[key] - whole1[key]) <= rtol * np.abs(whole1[key])), (key, np.abs(part1[key] - whole1[key]).max())
        assert np.all(np.abs(part2[key] - whole2[key]) <= 2 * rtol * np.abs(whole2[key])), key
    g.finalize_Integrator()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def _direct_call(g, source, nb=2, n=8):
    lay, play = B.MomentsLayout(), B.PathMomentsLayout()
    assert g._lib.i3rc_hip_get_moments_layout(g._h, C.byref(lay)) == 0 and g._lib.i3rc_hip_get_path_moments_layout(g._h, C.byref(play)) == 0
    bufs = [np.zeros(k, np.float64) for k in (lay.total, lay.total, B.NUM_COUNTERS, play.total, play.total)]
    return g._lib.i3rc_hip_run_batches_path_moments(g._h, SEED[0], SEED[1], nb, n, C.byref(source), *[b.ctypes.data_as(B.dp) for b in bufs]), bufs


def test_refusals():
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3)
    play = B.PathMomentsLayout()
    assert g._lib.i3rc_hip_get_path_moments_layout(g._h, C.byref(play)) != 0
    assert b"i3rc_hip_get_path_moments_layout: no path tally is switched on" in g._lib.i3rc_hip_last_error(g._h)
    with pytest.raises(M.I3RCError, match="no path tally is switched on"):
        g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 1000)
    s = B.Source()
    s.kind, s.solarMu, s.solarAzimuth = 0, K.SOURCE[0], K.SOURCE[1]
    dummy = np.zeros(4096, np.float64)
    p = dummy.ctypes.data_as(B.dp)
    assert g._lib.i3rc_hip_run_batches_path_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, p, p) != 0
    assert (WHO + ": no path tally is switched on").encode() in g._lib.i3rc_hip_last_error(g._h) and (dummy == 0).all()
    # with level fluxes on the new call refuses, and the diagnostic moments go on working
    g.specifyParameters(computeLevelFluxes=True)
    assert g._lib.i3rc_hip_run_batches_path_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, p, p) != 0
    assert (WHO + ": no path tally is switched on").encode() in g._lib.i3rc_hip_last_error(g._h) and (dummy == 0).all()
    x1, _, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, 2, *K.SOURCE, 1000)
    assert cnt["photons"] == 2000 and (x1["levelFluxDown"][-1] > 0).all()
    g.specifyParameters(computeLevelFluxes=False)

    g.specifyParameters(computePathLengths=True)
    assert g._lib.i3rc_hip_get_path_moments_layout(g._h, C.byref(play)) == 0
    assert (play.kind, play.nBins, play.nK) == (3, 0, 0) and play.total == B.path_moments_layout("paths", g.nx, g.ny)["total"] and play.histogramUp == -1
    with pytest.raises(M.I3RCError, match=WHO + ": .*must ask for non-negative number of photons"):
        g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 0)
    with pytest.raises(M.I3RCError, match=WHO + ": bad arguments"):
        g.computeRadiativeTransferPathMoments(SEED, 0, *K.SOURCE, 1000)
    assert g._lib.i3rc_hip_run_batches_path_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, None, p) != 0
    assert (WHO + ": bad arguments").encode() in g._lib.i3rc_hip_last_error(g._h)
    rng = np.random.default_rng(3)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (rng.random(8), rng.random(8), rng.random(8), -rng.uniform(0.2, 1, 8), rng.random(8))]
    explicit = B.Source()
    explicit.kind = 1
    explicit.x, explicit.y, explicit.z, explicit.mu, explicit.phi = [B.pf(a) for a in arrays]
    rc, bufs = _direct_call(g, explicit)
    assert rc != 0 and (WHO + ": Directional photon streams only").encode() in g._lib.i3rc_hip_last_error(g._h) and all((b == 0).all() for b in bufs)
    g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
    with pytest.raises(M.I3RCError, match=WHO + ": path lengths are tallied by flux launches only; radiance directions are set"):
        g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(computeIntensity=False)
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match=WHO + ": path lengths need ray tracing; max cross-section is in use"):
        g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(useRayTracing=True)
    # the old entry points go on refusing the kind, with their pinned words -- and now say where its statistics are
    with pytest.raises(M.I3RCError, match="i3rc_hip_get_diagnostic_moments_layout: path lengths have no batch statistics.*" + WHO):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    assert g._lib.i3rc_hip_run_batches_diagnostic_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, p, p) != 0
    assert b"i3rc_hip_run_batches_diagnostic_moments: path lengths have no batch statistics" in g._lib.i3rc_hip_last_error(g._h) and (dummy == 0).all()
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches_moments: path lengths are tallied by plain launches only"):
        g.computeRadiativeTransferBatchMoments(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="bad arguments"):
        B.diagnostic_moments_layout("paths", g.nx, g.ny, g.nz)

    # the spectrum's bad inputs, each by what is wrong with it; what was set stays
    g.specifyParameters(absorptionCoefficients=[0.0, 0.002])
    for bad, text in (([0.1, -0.5], r"absorption coefficients must not be negative; absorption\[1\] is"),
                      ([np.nan, 0.5], r"absorption coefficients must be finite; absorption\[0\] is not"),
                      ([0.1, np.inf], r"absorption coefficients must be finite; absorption\[1\] is not"),
                      (np.zeros(257), "0 <= nK <= 256 required.*got 257")):
        with pytest.raises(M.I3RCError, match="i3rc_hip_set_path_spectrum: " + text):
            g.specifyParameters(absorptionCoefficients=bad)
        assert np.array_equal(g.absorptionCoefficients, f32([0.0, 0.002]))
    assert g._lib.i3rc_hip_set_path_spectrum(g._h, 2, None) != 0 and b"null absorption coefficients" in g._lib.i3rc_hip_last_error(g._h)
    assert g._lib.i3rc_hip_get_path_moments_layout(g._h, C.byref(play)) == 0 and (play.kind, play.nK) == (3, 2)
    total = g.layout().total
    g.specifyParameters(absorptionCoefficients=np.zeros(256))       # (the most there may be; it moves no offset of the tally block)
    assert g.layout().total == total
    g.specifyParameters(absorptionCoefficients=[0.0, 0.002])
    # ... and the handle works afterwards: path lengths, then the histogram with the coefficients set before it was switched on
    s1, _, cnt = g.computeRadiativeTransferPathMoments(SEED, 2, *K.SOURCE, 1000)
    assert cnt["photons"] == 2000 and (s1["pathLengthDown"] > 0).all() and "spectrumUpLower" not in s1 and "pathHistogramUp" not in s1
    g.specifyParameters(computePathLengths=False)
    g.specifyParameters(pathHistogramEdges=f32(SEVEN_EDGES * 250.0))
    assert g._lib.i3rc_hip_get_path_moments_layout(g._h, C.byref(play)) == 0 and (play.kind, play.nBins, play.nK) == (4, 6, 2)
    assert {k: getattr(play, k) for k in B.PATH_MOMENTS_NAMES} == B.path_moments_layout("bins", g.nx, g.ny, 6, 2)
    with pytest.raises(M.I3RCError, match="i3rc_hip_get_diagnostic_moments_layout: the path histogram has no batch statistics.*" + WHO):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match=WHO + ": the path histogram needs ray tracing"):
        g.computeRadiativeTransferPathMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(useRayTracing=True)
    s1, _, cnt = g.computeRadiativeTransferPathMoments(SEED, 2, *K.SOURCE, 1000)
    assert cnt["photons"] == 2000 and s1["spectrumUpLower"].shape == (2,) and (s1["spectrumUpLower"] > 0).all() and "pathLengthUp" not in s1
    g.specifyParameters(absorptionCoefficients=None)                 # the spectrum off: the histogram's statistics alone
    s1, _, cnt = g.computeRadiativeTransferPathMoments(SEED, 2, *K.SOURCE, 1000)
    assert cnt["photons"] == 2000 and s1["spectrumUpLower"].shape == (0,) and s1["pathHistogramUp"].sum() > 0
    g.finalize_Integrator()


# ---- 7: the Fortran shell and the driver ---------------------------------------------------------------------------------------------
def test_shell_path_moments_equal_the_python_mirrors():
    import os

    from tests.test_fortran_shell import BUILD, ROOT, _need, _run as run_exe
    from tests.test_gpu_diagnostic_moments import _printed

    exe = _need(os.path.join(BUILD, "pathMomentsTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "path moments test done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for key, text in (("nothingyet   T", "reportPathMoments: no path moments have been computed."),
                      ("switchedoff  T", "no path tally is switched on"),
                      ("badspectrum  T", "specifyParameters: i3rc_hip_set_path_spectrum: absorption coefficients must not be negative; absorption[1] is"),
                      ("wrongshape   T", "reportPathMoments: pathLengthDownStats array is the wrong size"),
                      ("unavailable  T", "reportPathMoments: path histogram information not available"),
                      ("nodiagnostic T", "reportDiagnosticMoments: no diagnostic moments have been computed."),
                      ("switchedoff2 T", "reportPathMoments: the problem has changed since the moments were computed."),
                      ("otherkind    T", "reportPathMoments: the problem has changed since the moments were computed."),
                      ("unavailable2 T", "reportPathMoments: path length information not available"),
                      ("wrongbins    T", "reportPathMoments: pathHistogramPathDownStats array is the wrong size"),
                      ("wrongspectr  T", "reportPathMoments: spectrumUpUpperStats array is the wrong size"),
                      ("otherspectr  T", "reportPathMoments: the problem has changed since the moments were computed."),
                      ("forgotten    T", "reportPathMoments: no path moments have been computed.")):
        assert any(l.startswith(key) and text in l for l in lines), (key, r.stdout)
    nx, ny, nz, nb, n, nbins = 4, 2, 6, 6, 5000, 24
    ext = np.full((nz, ny, nx), f32(0.0002), np.float32)
    for k in range(2, 5):
        for j in range(ny):
            for i in range(nx):
                ext[k, j, i] = f32(0.004) * f32(1 + (i + 1 + j + 1) % 3)
    d = dict(xe=f32(500.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(500.0) * np.arange(ny + 1, dtype=np.float32),
             ze=np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0, 1000.0], np.float32), ext=ext, ssa=np.full_like(ext, f32(0.95)),
             pf=np.ones(ext.shape, np.int32))

    def rows(key, width):
        got = [l.split() for l in lines if l.startswith(key + " ")]
        assert got and all(len(row) == 3 + width for row in got), (key, got[:2])
        return {(int(row[1]), int(row[2])): np.array([float(v) for v in row[3:]]) for row in got}

    def same(shell, want, what):
        want = np.asarray(want, np.float64).ravel()
        assert shell.shape == want.shape and (np.abs(shell - want) <= _printed(want)).all(), (what, np.abs(shell - want).max())

    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, computePathLengths=True)
    s = g.computeRadiativeTransferPathMoments((7, 3), nb, 0.5, 30.0, n)
    assert s[2]["photons"] == nb * n and [int(l.split()[1]) for l in lines if l.startswith("batches ")] == [nb]
    mf = [float(v) for v in next(l for l in lines if l.startswith("meanflux ")).split()[1:]]
    for got, want in zip(mf, (s[0]["meanFluxUp"], s[1]["meanFluxUp"], s[0]["meanFluxDown"], s[1]["meanFluxDown"])):
        assert abs(got - want) <= _printed(want), (got, want)
    domain, mean, field = rows("domainpath", 4), rows("meanpath", 4), rows("pathfield", nx * ny)
    for m in (1, 2):
        # (the shell's order is the block's: Up, SquaredUp, Down, SquaredDown)
        same(domain[m, 0], [s[m - 1][k] for k in ("domainPathUp", "domainPathSquaredUp", "domainPathDown", "domainPathSquaredDown")], ("domainpath", m))
        same(mean[m, 0], [s[m - 1][k] for k in P.SCALARS[:4]], ("meanpath", m))
        for f, name in enumerate(PATH_NAMES):
            same(field[m, f + 1], s[m - 1][name], (name, m))
    assert (domain[1, 0] > 0).all()
    g.specifyParameters(computePathLengths=False)
    edges = np.zeros(nbins + 1, np.float32)
    edges[1] = 500.0
    for b in range(2, nbins + 1):                                 # the shell's own float32 arithmetic: one product per edge
        edges[b] = edges[b - 1] * f32(1.25)
    g.specifyParameters(pathHistogramEdges=edges, absorptionCoefficients=f32([1e-5, 1e-4, 1e-3]))
    s = g.computeRadiativeTransferPathMoments((7, 3), nb, 0.5, 30.0, n)
    bins, spectrum = rows("bins", nbins + 1), rows("spectrum", 3)
    for m in (1, 2):
        for f, (name, word) in enumerate(zip(BIN_NAMES, P.SPECTRUM)):
            same(bins[m, f + 1], s[m - 1][name], (name, m))
            same(spectrum[m, f + 1], s[m - 1][word], (word, m))
    assert np.count_nonzero(bins[1, 1]) > 8 and (spectrum[1, 1] > 0).all()
    g.finalize_Integrator()


DRIVER_EDGES = (0.0, 100.0, 250.0, 500.0, 1000.0, 2500.0)
DRIVER_KS = (0.0, 0.001, 0.01)
DRIVER_DECKS = {"paths": dict(algorithms=", computePathLengths = .true.", file_key="outputPathLengthFile", params=dict(computePathLengths=True)),
                "bins": dict(algorithms=", pathHistogramEdges = " + ", ".join(f"{e:.1f}" for e in DRIVER_EDGES) + ", absorptionCoefficients = " + ", ".join(f"{k}" for k in DRIVER_KS),
                             file_key="outputPathHistogramFile", params=dict(pathHistogramEdges=f32(DRIVER_EDGES), absorptionCoefficients=f32(DRIVER_KS)))}


def _check_driver_files(tmp_path, tag, kind, dom):
    from scipy.io import netcdf_file

    from tests.test_gpu_diagnostic_moments import _drivers_statistics

    g = M.new_Integrator(M.read_Domain(dom))
    g.specifyParameters(surfaceAlbedo=0.2, minInverseTableSize=10001, **DRIVER_DECKS[kind]["params"])
    s1, s2, cnt = g.computeRadiativeTransferPathMoments((11, 1), 8, 0.7, 25.0, 4000)      # the driver's seeds: (/ iseed, batch /), batch = 1 ...
    assert cnt["photons"] == 8 * 4000
    g.finalize_Integrator()
    f = netcdf_file(str(tmp_path / f"{tag}.nc"), "r", mmap=False)
    rows = [[float(v) for v in l.split()] for l in open(str(tmp_path / f"{tag}_{kind}.txt")) if not l.startswith("!")]

    def check_variable(name, key, dims):
        assert f.variables[name].dimensions == dims and f.variables[name + "_StdErr"].dimensions == dims, (name, f.variables[name].dimensions)
        mean, se, dmean, dse = _drivers_statistics(s1[key], s2[key], 8)
        got_mean, got_se = f.variables[name].data, f.variables[name + "_StdErr"].data
        assert got_mean.shape == mean.shape and (np.abs(got_mean - mean) <= dmean).all(), (name, np.abs(got_mean - mean).max())
        assert (np.abs(got_se - se) <= dse).all() and (got_se > 0).any(), (name, np.abs(got_se - se).max(), dse.max())

    def check_printed(got, keys, digits):
        """mean and StdErr pairs of a row against the mirror's sums (pairs of s1, s2 words): printed with four decimals (digits None),
        or with seven significant digits"""
        assert len(got) == 2 * len(keys)
        for col, (a1, a2) in enumerate(keys):
            mean, se, dmean, dse = _drivers_statistics(a1, a2, 8)
            for value, want, slack in ((got[2 * col], mean, dmean), (got[2 * col + 1], se, dse)):
                printed = 0.5001e-4 if digits is None else 0.5001e-6 * abs(float(want))
                assert abs(value - float(want)) <= printed + float(slack), (col, value, want, printed, slack)

    if kind == "paths":
        for name in PATH_NAMES:
            check_variable(name, name, ("y", "x"))
        assert len(rows) == 2 and "pathBin" not in f.dimensions and "pathHistogramUp" not in f.variables
        check_printed(rows[0], [(s1[k], s2[k]) for k in ("domainPathUp", "domainPathSquaredUp", "domainPathDown", "domainPathSquaredDown")], 7)
        check_printed(rows[1], [(s1[k], s2[k]) for k in P.SCALARS[:4]], 7)
        assert rows[0][0] > 0 and rows[0][1] > 0 and rows[0][4] > 0 and rows[0][5] > 0
    else:
        nb, nk = len(DRIVER_EDGES), len(DRIVER_KS)
        assert f.dimensions["pathBin"] == nb and f.dimensions["absorption"] == nk and "pathLengthUp" not in f.variables
        assert np.array_equal(f.variables["pathBinEdge"].data, f32(DRIVER_EDGES)) and np.array_equal(f.variables["absorptionCoefficient"].data, f32(DRIVER_KS))
        for name in BIN_NAMES:
            check_variable(name, name, ("pathBin",))
        for name in P.SPECTRUM:
            check_variable(name, name, ("absorption",))
        assert [len(r) for r in rows] == [10] * nb + [9] * nk, [len(r) for r in rows]
        for b in range(nb):
            assert rows[b][0] == DRIVER_EDGES[b] and rows[b][1] == (DRIVER_EDGES[b + 1] if b + 1 < nb else -1.0)
            check_printed(rows[b][2:4], [(s1["pathHistogramUp"][b], s2["pathHistogramUp"][b])], None)
            check_printed(rows[b][4:6], [(s1["pathHistogramPathUp"][b], s2["pathHistogramPathUp"][b])], 7)
            check_printed(rows[b][6:8], [(s1["pathHistogramDown"][b], s2["pathHistogramDown"][b])], None)
            check_printed(rows[b][8:10], [(s1["pathHistogramPathDown"][b], s2["pathHistogramPathDown"][b])], 7)
        for j in range(nk):
            assert abs(rows[nb + j][0] - DRIVER_KS[j]) <= 1e-6 * DRIVER_KS[j]
            check_printed(rows[nb + j][1:], [(s1[k][j], s2[k][j]) for k in P.SPECTRUM], None)
        assert rows[nb][1] > rows[nb + 2][1] > 0
    return f


@pytest.mark.parametrize("kind", list(DRIVER_DECKS))
def test_the_driver_reports_the_path_tally_with_its_standard_errors(kind, tmp_path):
    from tests.test_gpu_diagnostic_moments import _run_driver

    deck = DRIVER_DECKS[kind]
    dom, rc, out = _run_driver(tmp_path, "on", algorithms=deck["algorithms"], files=f', {deck["file_key"]} = "{tmp_path}/on_{kind}.txt"')
    assert rc == 0 and "Wrote ASCII figures of the path tally" in out and "Wrote ASCII results" in out and "Wrote netCDF results" in out, out
    _check_driver_files(tmp_path, "on", kind, dom)


def test_the_driver_ends_with_the_librarys_refusals_of_the_path_tallies(tmp_path):
    from tests.test_gpu_diagnostic_moments import _run_driver

    paths, bins = DRIVER_DECKS["paths"]["algorithms"], DRIVER_DECKS["bins"]["algorithms"]
    for tag, deck, text in (("both", dict(algorithms=paths + bins), "i3rc_hip_set_path_histogram: path lengths are switched on"),
                            ("levels", dict(algorithms=", computeLevelFluxes = .true." + paths), "i3rc_hip_set_path_lengths: level fluxes are switched on"),
                            ("radiance", dict(algorithms=paths, radiative=", intensityMus = 1., intensityPhis = 0."),
                             "path lengths are tallied by flux launches only; radiance directions are set"),
                            ("maxcross", dict(algorithms=bins, ray_tracing=".false."), "the path histogram needs ray tracing; max cross-section is in use"),
                            ("edges", dict(algorithms=", pathHistogramEdges = 0., 100., 100., 300."), "edges must be strictly ascending")):
        dom, rc, out = _run_driver(tmp_path, tag, **deck)
        out = out.replace("\n ", "")                      # (list-directed output breaks its lines at 80 characters)
        assert text in out and "Wrote" not in out, (tag, out)
        assert not (tmp_path / f"{tag}_flux.txt").exists() and not (tmp_path / f"{tag}.nc").exists(), tag


def _gpu_count():
    try:
        import torch

        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.skipif(_gpu_count() < 2, reason="needs two GPUs: the driver's batches split over two processes, one GPU each")
def test_two_processes_give_the_drivers_path_files_of_one(tmp_path):
    """the path moments travel in the one packed all-reduce of sumBatchMomentsAcrossProcesses: two processes with four batches each
    report what one process with eight reports"""
    from tests.test_gpu_diagnostic_moments import _run_driver

    deck = DRIVER_DECKS["bins"]
    dom, rc, out = _run_driver(tmp_path, "two", world=2, algorithms=deck["algorithms"], files=f', {deck["file_key"]} = "{tmp_path}/two_bins.txt"')
    assert rc == 0 and "batches on each of" in out, out
    _check_driver_files(tmp_path, "two", "bins", dom)
