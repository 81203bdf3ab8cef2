"""Batch statistics of the optional diagnostic tally on the device (i3rc_hip_run_batches_diagnostic_moments, through the mirror's
computeRadiativeTransferDiagnosticMoments): the level fluxes and the actinic flux of a loop's batches, normalised and added up -- x and
x^2, per element and per domain mean -- by moments_fields_kernel / moments_means_kernel over ExtraFields behind every batch's launch.

  the loop is its batches   s1, s2 against the same batches run one by one (computeRadiativeTransfer + reportResults, float64 sums on
                            the host), ordinary moments included, once per place of the extinction field and kind
  one batch, bit for bit    where a batch's sums do not depend on their order: s1 = float64(field), s2 = s1 s1, also on an irregular grid
  identities                levelFluxDown[0] = fluxDown, levelFluxUp[nz] = fluxUp, meanLevelFluxUp[nz] = meanFluxUp inside one call
  statistics                mean and standard error of every level's domain mean against tests/level_flux_solver.py
  launches                  more batches than slots, batches below a wavefront, split batches, a second call, the refusals

Tolerances.  The device adds the float32 values the host reports, in float64: 1e-9 on the sums of the fields, 2e-9 on those of their
squares; the domain means are a tree sum on the device against numpy's: 2e-6 and 4e-6 (test_batch_moments_on_the_device_equal_the_
drivers_sums, tests/test_gpu_parity.py).  Two float32 roundings of two float64 sums of the same increments differ by at most 2^-23 of
the value per batch.  Split batches: tests/sums.py, plus one float32 rounding of every batch's value."""
import ctypes as C
import os

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.extra_tally import IRREGULAR_Z, PLACES, run, step_cloud_3d
from tests.sums import F32_ULP, order_rtol
from tests.test_gpu_parity import hg_table, make_gpu

pytestmark = pytest.mark.gpu

B = M.binding
f32 = np.float32
SEED = (31, 8)
NB, N = 5, 3001
KINDS = {"levels": dict(switch="computeLevelFluxes", stream="PhiloxLevelStream", report=dict(levelFluxUp=True, levelFluxDown=True),
                        fields=("levelFluxUp", "levelFluxDown"), means=("meanLevelFluxUp", "meanLevelFluxDown")),
         "tracks": dict(switch="computeActinicFlux", stream="PhiloxTrackStream", report=dict(actinicFlux=True),
                        fields=("actinicFlux",), means=("meanActinicFlux",))}
MEAN_OF = {"meanLevelFluxUp": "levelFluxUp", "meanLevelFluxDown": "levelFluxDown", "meanActinicFlux": "actinicFlux"}


def one_by_one(g, kind, nb, n, seed=SEED, sun=K.SOURCE):
    """the loop's batches through computeRadiativeTransfer + reportResults: per-batch dicts of everything the moments hold (the
    diagnostic's domain means formed here: the plain mean over the columns, rounded once), and the counters summed"""
    per, counters = [], None
    for b in range(nb):
        res = run(g, n, seed=(seed[0], seed[1] + b), sun=sun)
        rep = dict(g.reportResults(**KINDS[kind]["report"]))
        for m in KINDS[kind]["means"]:
            rep[m] = np.float32(np.asarray(rep[MEAN_OF[m]], np.float64).mean(axis=(1, 2)))
        per.append(rep)
        counters = dict(res["counters"]) if counters is None else {k: counters[k] + v for k, v in res["counters"].items()}
    return per, counters


def assert_moments_are_the_batches(s1, s2, per, what):
    assert set(KINDS[what[0]]["fields"] + KINDS[what[0]]["means"]) <= set(s1) and set(s1) == set(s2), sorted(s1)
    for key in s1:
        x = np.stack([np.asarray(p[key], np.float64) for p in per])
        want1, want2 = x.sum(0), (x * x).sum(0)
        tol = 2e-6 if key.startswith("mean") or key == "absorbedProfile" else 1e-9
        print(what, key, "largest relative difference", float((np.abs(s1[key] - want1) / np.maximum(np.abs(want1), 1e-300)).max()), "allowed", tol)
        assert np.shape(s1[key]) == want1.shape, (what, key, np.shape(s1[key]), want1.shape)
        assert np.allclose(s1[key], want1, rtol=tol, atol=1e-12), (what, key, np.abs(s1[key] - want1).max())
        assert np.allclose(s2[key], want2, rtol=2 * tol, atol=1e-12), (what, key, np.abs(s2[key] - want2).max())


# ---- 1: the loop is its batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place,domain", PLACES, ids=[p for p, _ in PLACES])
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_loop_is_its_batches(kind, place, domain):
    """step_cloud_3d(0.9) wherever its field can lie (one component: LDS, linear, bricks, column records); records over a base profile
    need a second component: that place has the recipe's own domain (tests/extra_tally.py, PLACES)"""
    if place == "GRID_COLBASE":
        d, tabs = K.DOMAINS[domain]()
    else:
        d, tabs = step_cloud_3d(0.9), hg_table()
    g = make_gpu(d, tabs, surfaceAlbedo=0.3, **{KINDS[kind]["switch"]: True})
    g.select_grid_place(K.PLACE_KNOB[place])
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, NB, *K.SOURCE, N)
    assert g.kernel_name() == f"photon_kernel<{KINDS[kind]['stream']}, false, true, {place}>", g.kernel_name()
    per, counters = one_by_one(g, kind, NB, N)
    assert g.kernel_name() == f"photon_kernel<{KINDS[kind]['stream']}, false, true, {place}>", g.kernel_name()
    assert cnt == counters and cnt["photons"] == NB * N and cnt["scatterings"] > 0, (cnt, counters)
    assert_moments_are_the_batches(s1, s2, per, (kind, place))
    g.finalize_Integrator()


# ---- 2: one batch, bit for bit -----------------------------------------------------------------------------------------------------------
def _unequal_x(d):
    nx = len(d["xe"]) - 1
    xe = np.cumsum(np.concatenate([[0.0], 40.0 + 15.0 * (np.arange(nx) % 3)])).astype(np.float32)
    assert np.ptp(np.diff(xe)) > 1
    return dict(d, xe=xe)


@pytest.mark.parametrize("grid", ["regular", "irregular"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_batch_bit_for_bit(kind, grid):
    """levels: conservative scattering, no roulette, a black surface -- every weight is 1 and every level tally a whole number.  tracks:
    clear air under a zenith sun -- the steps in a cell all have one float32 length.  Either way a word's float64 sum does not depend
    on the order of its additions, two runs of a batch give one raw block, and host and kernel round it by one statement."""
    from tests.test_gpu_actinic_flux import _clear_domain

    if kind == "levels":
        d = step_cloud_3d(1.0)
        if grid == "irregular":
            d = _unequal_x(dict(d, ze=IRREGULAR_Z[:7]))
        g, sun = make_gpu(d, hg_table(), surfaceAlbedo=0.0, useRussianRoulette=False, computeLevelFluxes=True), K.SOURCE
    else:
        d = _clear_domain(8, 4, np.array([0.0, 30.1, 80.7, 120.3, 170.9, 210.2, 250.6], np.float32) if grid == "regular" else IRREGULAR_Z)
        if grid == "irregular":
            d = _unequal_x(d)
        g, sun = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeActinicFlux=True), (1.0, 0.0)
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, 1, *sun, N)
    (want,), counters = one_by_one(g, kind, 1, N, sun=sun)
    assert cnt == counters and cnt["photons"] == N and cnt["dropped"] == 0 and cnt["roulette"] == 0
    for key in KINDS[kind]["fields"]:
        w = np.asarray(want[key], np.float64)
        assert w.max() > 0 and len(np.unique(want[key])) > 4, key
        assert np.array_equal(s1[key].view(np.uint64), w.view(np.uint64)), (key, np.argwhere(s1[key] != w)[:8])
        assert np.array_equal(s2[key].view(np.uint64), (w * w).view(np.uint64)), key
    g.finalize_Integrator()


# ---- 3: identities inside one call -------------------------------------------------------------------------------------------------------
def test_boundary_levels_are_the_boundary_fluxes():
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3, computeLevelFluxes=True)
    s1, _, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, NB, *K.SOURCE, N)
    nz = g.nz
    for a, b, what in ((s1["levelFluxDown"][0], s1["fluxDown"], "levelFluxDown[0] = fluxDown"), (s1["levelFluxUp"][nz], s1["fluxUp"], "levelFluxUp[nz] = fluxUp"),
                       (s1["meanLevelFluxUp"][nz], s1["meanFluxUp"], "meanLevelFluxUp[nz] = meanFluxUp"),
                       (s1["meanLevelFluxDown"][0], s1["meanFluxDown"], "meanLevelFluxDown[0] = meanFluxDown")):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        print(what, "largest |difference| / |s1|", float((np.abs(a - b) / np.abs(b)).max()), "allowed", NB * F32_ULP)
        assert np.all(b > 0) and np.all(np.abs(a - b) <= NB * F32_ULP * np.abs(b)), (what, np.abs(a - b).max())
    g.finalize_Integrator()


# ---- 4: the statistics are usable --------------------------------------------------------------------------------------------------------
def test_level_means_and_their_standard_errors_against_the_solver():
    """Every level's domain mean within 4 of ITS OWN reported standard errors (+ 3e-5: what the solver does not model,
    tests/test_plane_parallel.py) of the adding solver; mean and standard error from s1, s2 as the drivers form them (real(4):
    m = s / nb, se = sqrt(max(0, m2 - m1^2) / (nb - 1))).  Every standard error is positive and below 0.01 -- but for the one quantity
    that has none: the downward flux through the top of the domain is the incident flux, 1 in every batch, which is asserted exactly."""
    from tests.level_flux_solver import solve_levels
    from tests.test_plane_parallel import G, MOMENTS, MU0, SIGMAS, MODEL, _sampled_moments
    from tools import cases

    tau, omega, albedo, nb, n = 1.0, 0.9, 0.5, 20, 50_000
    assert SIGMAS == 4 and MODEL == 3e-5
    d = cases.plane_parallel(optical_depth=tau, ssa=omega, nx=2, ny=2, nlayers=8)
    g = make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, computeLevelFluxes=True)
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments((10, 1), nb, MU0, 0.0, n)
    assert cnt["photons"] == nb * n
    depth = tau * (1.0 - np.arange(9) / 8.0)                       # optical depth above level k
    want_up, want_down = solve_levels(depth, tau, omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    for name, want in (("meanLevelFluxUp", want_up), ("meanLevelFluxDown", want_down)):
        m1, m2 = f32(s1[name]) / f32(nb), f32(s2[name]) / f32(nb)
        se = np.sqrt(np.maximum(f32(0), m2 - m1 * m1) / f32(nb - 1))
        print(name, "mean - solver", m1 - want, "standard errors", se, "largest |difference| / (4 se + 3e-5)", float((np.abs(m1 - want) / (SIGMAS * se + MODEL)).max()))
        assert (np.abs(m1 - want) <= SIGMAS * se + MODEL).all(), (name, m1 - want, se)
        random = np.ones(9, bool)
        if name == "meanLevelFluxDown":
            # the downward flux through the TOP is no random variable: every photon of a Directional source comes in there, the domain
            # mean is 1 in every batch -- exactly -- and its standard error is 0 (measured: 0.0; the other levels 1.9e-4 ... 2.7e-4)
            random[8] = False
            assert s1[name][8] == nb and s2[name][8] == nb and se[8] == 0, (s1[name][8], s2[name][8], se[8])
        assert (se[random] > 0).all() and (se < 0.01).all(), (name, se)
    g.finalize_Integrator()


# ---- 5: launch mechanics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_more_batches_than_slots_small_batches_and_a_second_call(kind):
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3, **{KINDS[kind]["switch"]: True})
    for nb, n in ((7, N), (7, 1), (3, 63)):        # 7 batches: one more than the slots; a batch of one photon; a batch below a wavefront
        s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, nb, *K.SOURCE, n)
        per, counters = one_by_one(g, kind, nb, n)
        assert cnt == counters and cnt["photons"] == nb * n
        assert_moments_are_the_batches(s1, s2, per, (kind, nb, n))
    # (each call above started from zeroed moments: a loop of 7 batches, then shorter ones); and the same call again gives the same sums
    t1, t2, _ = g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 63)
    for key in KINDS[kind]["fields"] + KINDS[kind]["means"]:
        assert np.allclose(t1[key], s1[key], rtol=1e-12, atol=0) and np.allclose(t2[key], s2[key], rtol=1e-12, atol=0), key
    g.finalize_Integrator()


@pytest.mark.parametrize("kind", list(KINDS))
def test_split_batches_give_the_unsplit_sums(kind):
    """i3rc_hip_set_launch_limit cuts every batch into launches of 1000 photons: the same increments in another order (tests/sums.py) in
    every raw word, then one float32 rounding per batch that may fall to the neighbour"""
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3, **{KINDS[kind]["switch"]: True})
    whole1, whole2, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, NB, *K.SOURCE, N)
    launches = g.timed_launches()
    assert B.load().i3rc_hip_set_launch_limit(g._h, 1000) == 0
    part1, part2, cnt2 = g.computeRadiativeTransferDiagnosticMoments(SEED, NB, *K.SOURCE, N)
    assert g.timed_launches() - launches == NB * 4 and cnt2 == cnt
    assert B.load().i3rc_hip_set_launch_limit(g._h, 0) == 0
    events = dict(cnt, photons=cnt["photons"] + cnt["cellSteps"])      # (a track-length word takes an addition per voxel step: tests/test_gpu_actinic_flux.py)
    rtol = order_rtol(events) + F32_ULP
    for key in KINDS[kind]["fields"]:
        assert np.all(np.abs(part1[key] - whole1[key]) <= rtol * np.abs(whole1[key])), (key, np.abs(part1[key] - whole1[key]).max())
        assert np.all(np.abs(part2[key] - whole2[key]) <= 2 * rtol * np.abs(whole2[key])), key
    g.finalize_Integrator()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    who = "i3rc_hip_run_batches_diagnostic_moments"
    g = make_gpu(step_cloud_3d(0.9), hg_table(), surfaceAlbedo=0.3)
    with pytest.raises(M.I3RCError, match=who + ": no diagnostic tally is switched on"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(computeLevelFluxes=True)
    with pytest.raises(M.I3RCError, match=who + ": .*must ask for non-negative number of photons"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 0)
    with pytest.raises(M.I3RCError, match=who + ": bad arguments"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 0, *K.SOURCE, 1000)
    lay, xlay = B.MomentsLayout(), B.DiagnosticMomentsLayout()
    assert g._lib.i3rc_hip_get_moments_layout(g._h, C.byref(lay)) == 0 and g._lib.i3rc_hip_get_diagnostic_moments_layout(g._h, C.byref(xlay)) == 0
    assert xlay.kind == 1 and xlay.total == B.diagnostic_moments_layout("levels", g.nx, g.ny, g.nz)["total"]
    bufs = [np.zeros(n, np.float64) for n in (lay.total, lay.total, B.NUM_COUNTERS, xlay.total, xlay.total)]
    rng = np.random.default_rng(3)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (rng.random(8), rng.random(8), rng.random(8), -rng.uniform(0.2, 1, 8), rng.random(8))]
    s = B.Source()
    s.kind = 1
    s.x, s.y, s.z, s.mu, s.phi = [B.pf(a) for a in arrays]
    assert g._lib.i3rc_hip_run_batches_diagnostic_moments(g._h, SEED[0], SEED[1], 2, 8, C.byref(s), *[b.ctypes.data_as(B.dp) for b in bufs]) != 0
    assert (who + ": Directional photon streams only").encode() in g._lib.i3rc_hip_last_error(g._h)
    g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
    with pytest.raises(M.I3RCError, match=who + ": level fluxes are tallied by flux launches only; radiance directions are set"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(computeIntensity=False)
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match=who + ": level fluxes need ray tracing; max cross-section is in use"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(useRayTracing=True, computeLevelFluxes=False)
    g.specifyParameters(computeActinicFlux=True)
    assert g._lib.i3rc_hip_get_diagnostic_moments_layout(g._h, C.byref(xlay)) == 0 and xlay.kind == 2 and xlay.levelFluxUp == -1
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match=who + ": the actinic flux needs ray tracing"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    g.specifyParameters(useRayTracing=True)
    s1, _, cnt = g.computeRadiativeTransferDiagnosticMoments(SEED, 2, *K.SOURCE, 1000)      # ... and the handle works afterwards
    assert cnt["photons"] == 2000 and (s1["actinicFlux"] > 0).all() and "levelFluxUp" not in s1
    g.finalize_Integrator()


# ---- 7: the Fortran shell and the driver ---------------------------------------------------------------------------------------------
def _printed(x):
    """what a real(4) printed with es16.8 (nine significant digits) can be off by: the conversion float64 -> real(4), and the print"""
    return np.abs(x) * (2.0 ** -24 + 0.6e-8)


def test_shell_moments_equal_the_python_mirrors():
    from tests.test_fortran_shell import BUILD, ROOT, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "diagnosticMomentsTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "diagnostic moments test done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for key, text in (("nothingyet   T", "reportDiagnosticMoments: no diagnostic moments have been computed."),
                      ("switchedoff  T", "i3rc_hip_run_batches_diagnostic_moments: no diagnostic tally is switched on"),
                      ("wrongshape   T", "reportDiagnosticMoments: levelFluxUpStats array is the wrong size"),
                      ("wrongmean    T", "reportDiagnosticMoments: meanLevelFluxDownStats array is the wrong size"),
                      ("unavailable  T", "reportDiagnosticMoments: actinic flux information not available"),
                      ("switchedoff2 T", "reportDiagnosticMoments: the problem has changed since the moments were computed."),
                      ("otherkind    T", "reportDiagnosticMoments: the problem has changed since the moments were computed."),
                      ("unavailable2 T", "reportDiagnosticMoments: level flux information not available"),
                      ("forgotten    T", "reportDiagnosticMoments: no diagnostic moments have been computed.")):
        assert any(l.startswith(key) and text in l for l in lines), (key, r.stdout)
    nx, ny, nz, nb, n = 4, 2, 6, 6, 5000
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
        assert all(len(row) == 3 + width for row in got), (key, got[:2])
        return {m: np.array([[float(v) for v in row[3:]] for row in got if int(row[1]) == m]) for m in (1, 2)}

    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, computeLevelFluxes=True)
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments((7, 3), nb, 0.5, 30.0, n)
    assert cnt["photons"] == nb * n and [int(l.split()[1]) for l in lines if l.startswith("batches ")] == [nb]
    mf = [float(v) for v in next(l for l in lines if l.startswith("meanflux ")).split()[1:]]
    for got, want in zip(mf, (s1["meanFluxUp"], s2["meanFluxUp"], s1["meanFluxDown"], s2["meanFluxDown"])):
        assert abs(got - want) <= _printed(want), (got, want)
    for key, name, width in (("meanup", "meanLevelFluxUp", 1), ("meandown", "meanLevelFluxDown", 1), ("levelup", "levelFluxUp", nx * ny), ("leveldown", "levelFluxDown", nx * ny)):
        shell = rows(key, width)
        for m, want in ((1, s1[name]), (2, s2[name])):
            want = np.asarray(want).reshape(nz + 1, width)
            assert shell[m].shape == want.shape and (np.abs(shell[m] - want) <= _printed(want)).all(), (key, m, np.abs(shell[m] - want).max())
    g.specifyParameters(computeLevelFluxes=False)
    g.specifyParameters(computeActinicFlux=True)
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments((7, 3), nb, 0.5, 30.0, n)
    for key, name, width in (("meanactinic", "meanActinicFlux", 1), ("actinic", "actinicFlux", nx * ny)):
        shell = rows(key, width)
        for m, want in ((1, s1[name]), (2, s2[name])):
            want = np.asarray(want).reshape(nz, width)
            assert shell[m].shape == want.shape and (np.abs(shell[m] - want) <= _printed(want)).all(), (key, m, np.abs(shell[m] - want).max())
    g.finalize_Integrator()


def _deck(dom, out, tag, algorithms="", files="", radiative="", ray_tracing=".true."):
    return f"""&radiativeTransfer
  solarFlux = 1., solarMu = 0.7, solarAzimuth = 25., surfaceAlbedo = 0.2{radiative} /
&monteCarlo
  numPhotonsPerBatch = 4000, numBatches = 8, iseed = 11, nPhaseIntervals = 10001 /
&algorithms
  useRayTracing = {ray_tracing}, useRussianRoulette = .true.{algorithms} /
&output
  reportVolumeAbsorption = .true., reportAbsorptionProfile = .true. /
&fileNames
  domainFileName = "{dom}", outputFluxFile = "{out}/{tag}_flux.txt", outputAbsProfFile = "{out}/{tag}_prof.txt",
  outputAbsVolumeFile = "{out}/{tag}_vol.txt", outputNetcdfFile = "{out}/{tag}.nc"{files} /
"""


def _drivers_statistics(s1, s2, nb):
    """mean and standard error as i3rcDriver forms them, in real(4) (solarFlux = 1): m = s / nb, se = sqrt(max(0, m2 - m1^2) / (nb - 1));
    and what the driver's own real(4) arithmetic may move them by: a rounding of m1, and for the standard error -- the square root of
    a small difference of two nearly equal numbers -- 2^-22 of the larger of them (m2 and m1^2 rounded, the product fused or not)"""
    m1, m2 = f32(1.0) * np.float32(s1) / f32(nb), f32(1.0) * np.float32(s2) / f32(nb)
    var = np.maximum(f32(0), m2 - m1 * m1) / f32(nb - 1)
    se = np.sqrt(var)
    dvar = 2.0 ** -22 * np.maximum(m2, m1 * m1).astype(np.float64) / (nb - 1)
    dse = np.sqrt(var.astype(np.float64) + dvar) - np.sqrt(np.maximum(var.astype(np.float64) - dvar, 0.0)) + 2.0 ** -23 * se
    return m1, se, 2.0 ** -23 * np.abs(m1), dse


def _run_driver(tmp_path, tag, world=1, **deck):
    from tests.test_fortran_shell import BUILD, ROOT, _need, _run as run_exe, _spawn_ranks

    drv, mk = _need(os.path.join(BUILD, "i3rcDriver")), _need(os.path.join(BUILD, "makeStepCloudDomain"))
    dom = str(tmp_path / "stepCloud.dom")
    if not os.path.exists(dom):
        assert run_exe([mk, dom, "8", "0.9"]).returncode == 0
    nml = tmp_path / f"{tag}.nml"
    nml.write_text(_deck(dom, tmp_path, tag, **deck))
    if world == 1:
        r = run_exe([drv, str(nml)], cwd=ROOT)
        return dom, r.returncode, r.stdout + r.stderr
    rcs, outs = _spawn_ranks([drv, str(nml)], world, 29661, cwd=ROOT)
    return dom, max(rcs), "\n".join(outs)


def _mirror_of_the_deck(dom, switch):
    g = M.new_Integrator(M.read_Domain(dom))
    g.specifyParameters(surfaceAlbedo=0.2, minInverseTableSize=10001, **{switch: True})
    s1, s2, cnt = g.computeRadiativeTransferDiagnosticMoments((11, 1), 8, 0.7, 25.0, 4000)      # the driver's seeds: (/ iseed, batch /), batch = 1 ...
    assert cnt["photons"] == 8 * 4000
    g.finalize_Integrator()
    return s1, s2


def _check_driver_files(tmp_path, tag, kind, dom):
    from scipy.io import netcdf_file

    s1, s2 = _mirror_of_the_deck(dom, KINDS[kind]["switch"])
    f = netcdf_file(str(tmp_path / f"{tag}.nc"), "r", mmap=False)
    nz = s1["volumeAbsorption"].shape[0]
    for name in KINDS[kind]["fields"]:
        want_dims = ("zLevel" if kind == "levels" else "z", "y", "x")       # (the file's order: the shell writes (x, y, z) column-major)
        assert f.variables[name].dimensions == want_dims and f.variables[name + "_StdErr"].dimensions == want_dims, f.variables[name].dimensions
        mean, se, dmean, dse = _drivers_statistics(s1[name], s2[name], 8)
        got_mean, got_se = f.variables[name].data, f.variables[name + "_StdErr"].data
        assert got_mean.shape == mean.shape and (np.abs(got_mean - mean) <= dmean).all(), (name, np.abs(got_mean - mean).max())
        assert (np.abs(got_se - se) <= dse).all(), (name, np.abs(got_se - se).max(), dse.max())
    if kind == "levels":
        assert f.dimensions["zLevel"] == nz + 1 and f.variables["zLevel"].data.shape == (nz + 1,)
    # the ASCII profile: height, then mean and StdErr of every domain mean, four decimals
    rows = [l.split() for l in open(str(tmp_path / f"{tag}_{kind}.txt")) if not l.startswith("!")]
    table = np.array([[float(v) for v in row] for row in rows])
    assert table.shape == ((nz + 1, 5) if kind == "levels" else (nz, 3)), table.shape
    for col, name in enumerate(KINDS[kind]["means"]):
        mean, se, dmean, dse = _drivers_statistics(s1[name], s2[name], 8)
        assert (np.abs(table[:, 1 + 2 * col] - mean) <= 0.5001e-4 + dmean).all(), (name, table[:, 1 + 2 * col] - mean)
        assert (np.abs(table[:, 2 + 2 * col] - se) <= 0.5001e-4 + dse).all(), (name, table[:, 2 + 2 * col] - se)
    assert (table[:, 1] > 0).all() and (table[:, 2] > 0).all()
    return f


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_driver_reports_the_diagnostic_with_its_standard_errors(kind, tmp_path):
    switch = KINDS[kind]["switch"]
    file_key = "outputLevelFluxFile" if kind == "levels" else "outputActinicFluxFile"
    dom, rc, out = _run_driver(tmp_path, "on", algorithms=f", {switch} = .true.", files=f', {file_key} = "{tmp_path}/on_{kind}.txt"')
    assert rc == 0 and "Wrote ASCII results" in out and "Wrote netCDF results" in out, out
    f = _check_driver_files(tmp_path, "on", kind, dom)
    other = KINDS["tracks" if kind == "levels" else "levels"]["fields"]
    assert not any(name in f.variables for name in other)
    if kind == "tracks":
        assert "cells without extinction" in open(str(tmp_path / f"on_{kind}.txt")).read()


def test_the_driver_without_the_switches_writes_what_it_wrote(tmp_path):
    """the deck with the two switches absent and with both .false. (and file names given for their profiles): every ASCII file byte for
    byte, the netCDF file variable for variable and attribute for attribute -- but for the two CPU times it records --, no new variable"""
    from scipy.io import netcdf_file

    tmp = tmp_path
    dom, rc, out = _run_driver(tmp, "absent")
    assert rc == 0 and "Wrote netCDF results" in out, out
    off = ', computeLevelFluxes = .false., computeActinicFlux = .false.'
    dom, rc, out = _run_driver(tmp, "off", algorithms=off, files=f', outputLevelFluxFile = "{tmp}/off_levels.txt", outputActinicFluxFile = "{tmp}/off_tracks.txt"')
    assert rc == 0 and "Wrote netCDF results" in out and "diagnostic" not in out, out
    assert not (tmp / "off_levels.txt").exists() and not (tmp / "off_tracks.txt").exists()
    for name in ("flux", "prof", "vol"):
        a, b = (tmp / f"absent_{name}.txt").read_bytes(), (tmp / f"off_{name}.txt").read_bytes()
        assert len(a) > 200 and a == b, name
    fa, fo = netcdf_file(str(tmp / "absent.nc"), "r", mmap=False), netcdf_file(str(tmp / "off.nc"), "r", mmap=False)
    assert list(fa.variables) == list(fo.variables) and list(fa.dimensions.items()) == list(fo.dimensions.items())
    assert list(fa.variables) == ["x", "y", "z", "fluxUp", "fluxUp_StdErr", "fluxDown", "fluxDown_StdErr", "fluxAbsorbed", "fluxAbsorbed_StdErr",
                                  "absorptionProfile", "absorptionProfile_StdErr", "absorbedVolume", "absorbedVolume_StdErr"]
    for k in fa.variables:
        assert fa.variables[k].dimensions == fo.variables[k].dimensions and fa.variables[k].data.tobytes() == fo.variables[k].data.tobytes(), k
    assert list(fa._attributes) == list(fo._attributes)
    for k in fa._attributes:
        if not k.startswith("Cpu_time"):
            assert np.all(fa._attributes[k] == fo._attributes[k]), k
    assert os.path.getsize(str(tmp / "absent.nc")) == os.path.getsize(str(tmp / "off.nc"))


def test_the_driver_ends_with_the_librarys_refusals(tmp_path):
    both = ", computeLevelFluxes = .true., computeActinicFlux = .true."
    for tag, deck, text in (("both", dict(algorithms=both), "i3rc_hip_set_actinic_flux: level fluxes are switched on"),
                            ("radiance", dict(algorithms=", computeLevelFluxes = .true.", radiative=", intensityMus = 1., intensityPhis = 0."),
                             "level fluxes are tallied by flux launches only; radiance directions are set"),
                            ("maxcross", dict(algorithms=", computeActinicFlux = .true.", ray_tracing=".false."),
                             "the actinic flux needs ray tracing; max cross-section is in use")):
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
def test_two_processes_give_the_drivers_files_of_one(tmp_path):
    """the diagnostic moments travel in the one packed all-reduce of sumBatchMomentsAcrossProcesses: two processes with four batches
    each report what one process with eight reports"""
    dom, rc, out = _run_driver(tmp_path, "two", world=2, algorithms=", computeLevelFluxes = .true.", files=f', outputLevelFluxFile = "{tmp_path}/two_levels.txt"')
    assert rc == 0 and "batches on each of" in out, out
    _check_driver_files(tmp_path, "two", "levels", dom)
