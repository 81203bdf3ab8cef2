"""Path-length moments of local-estimate radiances on the device: the block of 2 nDir nx ny float64 words that
photon_kernel<PhiloxRadiancePathStream, true, true, GRID> fills -- per radiance direction and column the sums of c L and c L^2 over the
contributions c the launch adds to that radiance, L the photon's path to the event plus the ray's straight way to the top -- and its
normalised form.

  exact            an empty domain over a Lambertian surface: every contribution of a direction has the same L = H (1 / mu0 + 1 / mu)
  same photons     against the side build whose general kernels run the same nested local estimate without the tally
                   (-DI3RC_NESTED_BUILD, in a child process): every counter identical, every old tally to the order of its float64
                   additions (tests/sums.py)
  launches         split batches, zeroing, a change of nDir, the refusals
  solver           <L> and <L^2> of a slab's radiances against the derivatives of the adding-doubling solver in a gas absorber
  3-D              the equivalence theorem as an inequality against radiance runs of the ray-queue kernels with a real absorber

Tolerances.  Exact: (nz + 3) 2^-23 relative on <L> -- the path is at most nz + 1 float32 pieces added in float64, one float32 start
height, the float32 rounding of the output -- and twice that on <L^2>.  Same photons: tests/sums.py.  Solver: 4 batch standard errors
plus the solver's own |Richardson value - central difference at 1e-3|.  3-D: the bracket widened by 4 combined batch standard errors
in the domain mean, the excursion allowance of tests.test_gpu_parity._assert_3sigma per column."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests.plane_parallel_solver import solve
from tests.sums import assert_same_sums
from tests.test_gpu_parity import hg_table, make_gpu
from tools import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RRI = dict(useRussianRouletteForIntensity=True, zetaMin=0.3)
N = 20_000


def _run(g, seed, n=N, sun=(0.5, 25.0)):
    return g.computeRadiativeTransfer(M.new_RandomNumberSequence(seed), M.new_PhotonStream(sun[0], sun[1], n))


def _block(g, res):
    """the two raw fields as (nDir, ny, nx) views of a result's packed buffer"""
    p1, p2, total = g.radiance_path_length_layout()
    nd, ncol = len(g.intensityDirections), g.ny * g.nx
    first = g.layout().counters + M.binding.NUM_COUNTERS
    assert (p1, p2, total) == (first, first + nd * ncol, first + 2 * nd * ncol) and total == len(res["raw"]) == g.layout().total, (p1, p2, total)
    return [res["raw"][at:at + nd * ncol].reshape(nd, g.ny, g.nx) for at in (p1, p2)]


# ---- 1: exact -------------------------------------------------------------------------------------------------------------------------
EMPTY_Z = np.array([0.0, 0.125, 0.5, 0.625, 1.25, 2.0], np.float32)      # five irregular layers, H = 2
VIEW_MUS, VIEW_PHIS = [1.0, 0.5, 0.1], [0.0, 140.0, 310.0]               # nadir; a slant view; rays that cross the domain some seven times


def _empty_domain():
    nx, ny, nz = 4, 3, len(EMPTY_Z) - 1
    cells = (nz, ny, nx)
    return dict(xe=f32(0.75) * np.arange(nx + 1, dtype=np.float32), ye=f32(0.875) * np.arange(ny + 1, dtype=np.float32), ze=EMPTY_Z,
                ext=np.zeros(cells, np.float32), ssa=np.zeros(cells, np.float32), pf=np.zeros(cells, np.int32))


@pytest.mark.parametrize("rri", [False, True], ids=["plain", "roulette"])
def test_every_contribution_over_an_empty_domain_has_the_same_path(rri):
    d = _empty_domain()
    mu0, nz, H = 0.5, len(EMPTY_Z) - 1, float(EMPTY_Z[-1])
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.5, intensityMus=VIEW_MUS, intensityPhis=VIEW_PHIS, computeRadiancePathLengths=True,
                 **(RRI if rri else {}))
    res = _run(g, (71, 3), sun=(mu0, 25.0))
    assert g.kernel_name() == "photon_kernel<PhiloxRadiancePathStream, true, true, GRID_LDS>", g.kernel_name()
    c = res["counters"]
    assert c["photons"] == N and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == N and c["exitsTop"] == N, c
    # (the rays of mu = 0.1 run 9.95 H sideways: several widths of the domain)
    assert H * np.sqrt(1 - 0.1 ** 2) / 0.1 > 5 * float(d["xe"][-1])
    inten = res["intensity"].astype(np.float64)
    p1, p2 = res["radiancePathLength"].astype(np.float64), res["radiancePathLengthSquared"].astype(np.float64)
    assert inten.shape == p1.shape == p2.shape == (3, g.ny, g.nx) and res["radiancePathLength"].dtype == np.float32
    assert (inten.sum(axis=(1, 2)) > 0).all()
    bound = (nz + 3) * 2.0 ** -23
    for k, mu in enumerate(np.float32(VIEW_MUS).astype(np.float64)):       # (the cosine the kernel divides by is the float32 one)
        has = inten[k] > 0
        assert has.any() and (p1[k][~has] == 0).all() and (p2[k][~has] == 0).all()
        L = H * (1.0 / mu0 + 1.0 / mu)
        e1 = np.abs(p1[k][has] / inten[k][has] / L - 1.0).max()
        e2 = np.abs(p2[k][has] / inten[k][has] / (L * L) - 1.0).max()
        print("direction", k, "mu", mu, "L", L, "columns", int(has.sum()), "errors in units of 2^-23:", e1 * 2.0 ** 23, e2 * 2.0 ** 23)
        assert e1 <= bound, (k, e1, bound)
        assert e2 <= 2 * bound, (k, e2, 2 * bound)
    # the raw block: what the normalised fields are made of, and nothing of it without a radiance
    b1, b2 = _block(g, res)
    assert (b1 > 0).any() and ((b1 > 0) == (b2 > 0)).all()
    g.finalize_Integrator()


# ---- 2: the same photons as the nested build --------------------------------------------------------------------------------------------
def _irregular_two_components():
    d = cases.step_cloud(ssa=0.95, nlayers=8, ncolumns=8)
    xe = np.array([0.0, 40.0, 110.0, 170.0, 250.0, 300.0, 390.0, 430.0, 500.0], np.float32)
    ze = np.array([0.0, 12.0, 40.0, 47.0, 90.0, 131.0, 160.0, 233.0, 250.0], np.float32)
    gas = np.full_like(d["ext"], f32(0.002))
    return dict(xe=xe, ye=d["ye"], ze=ze, ext=[d["ext"], gas], ssa=[d["ssa"], np.full_like(gas, f32(0.6))], pf=[d["pf"], d["pf"]])


def _parity_cases():
    """(domain, tables, parameters) -- the child process builds the same"""
    two = dict(RRI, intensityMus=[1.0, 0.45], intensityPhis=[0.0, 200.0], surfaceAlbedo=0.3)
    surface = M.new_SurfaceDescription(np.array([[0.1, 0.6], [0.4, 0.2]], f32), np.array([0.0, 200.0, 500.0], f32), np.array([0.0, 300.0, 500.0], f32))
    return {
        "step cloud": (cases.step_cloud(ssa=0.95, nlayers=8, ncolumns=8), hg_table(), two),
        "irregular, two components": (_irregular_two_components(), [hg_table(), hg_table(0.0, 8)], two),
        "gridded surface": (cases.step_cloud(ssa=1.0, nlayers=8, ncolumns=8), hg_table(), dict(intensityMus=[0.8], intensityPhis=[70.0], surfaceBDRF=surface)),
    }


def _parity_run(name, paths):
    d, tabs, kw = _parity_cases()[name]
    g = make_gpu(d, tabs, **kw)
    if paths:
        g.specifyParameters(computeRadiancePathLengths=True)
    else:
        g.set_tuning(forceGeneral=True)
    res = _run(g, (83, 5), sun=(0.6, 35.0))
    out = res["raw"][:g.layout().counters].copy(), res["counters"], g.kernel_name(), res
    return g, out


CHILD = r"""
import json, os, sys
sys.path.insert(0, %r)
import numpy as np
import i3rc_monte_carlo_model_amd as M
M.build.LIB = os.environ["I3RC_LIB"]; M.build.needs_build = lambda: False
from tests import test_gpu_radiance_path_lengths as T
out = {}
for name in T._parity_cases():
    g, (old, counters, kernel, _) = T._parity_run(name, False)
    np.save(os.path.join(sys.argv[1], name.replace(" ", "_").replace(",", "") + ".npy"), old)
    out[name] = [counters, kernel]
    g.finalize_Integrator()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def nested(tmp_path_factory):
    """the three cases through the nested-order side build's general radiance kernel, once, in a process of its own"""
    lib = M.build.build_variant("nested", M.build.NESTED_FLAGS)
    where = tmp_path_factory.mktemp("nested")
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(where)], capture_output=True, text=True, timeout=280, env=dict(os.environ, I3RC_LIB=lib))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    meta = json.loads(p.stdout.strip().splitlines()[-1])
    return {name: (np.load(os.path.join(where, name.replace(" ", "_").replace(",", "") + ".npy")), meta[name][0], meta[name][1]) for name in meta}


@pytest.mark.parametrize("name", ["step cloud", "irregular, two components", "gridded surface"])
def test_same_photons_as_the_nested_build(nested, name):
    """the feature draws no deviate and changes no decision"""
    want, counters, kernel = nested[name]
    assert kernel.startswith("photon_kernel<PhiloxStream, true, true, GRID_"), kernel
    g, (old, got, name_on, res) = _parity_run(name, True)
    assert name_on == kernel.replace("PhiloxStream", "PhiloxRadiancePathStream"), (name_on, kernel)
    assert got == counters and got["photons"] == N and got["scatterings"] > 0 and got["shadowSteps"] > 0, (got, counters)
    nd = len(g.intensityDirections)
    assert_same_sums(old, want, got, directions=nd, what=name)
    b1, b2 = _block(g, res)
    # Cauchy-Schwarz over the components' sum, word for word: (sum c L)^2 <= (sum c)(sum c L^2)
    lay = g.layout()
    by_comp = res["raw"][lay.intensityByComponent:lay.intensityExcess].reshape(g.ncomp + 1, nd, g.ny, g.nx)
    tot = by_comp.sum(axis=0)
    assert (tot > 0).all() and (b1 > 0).all() and (b2 > 0).all()
    assert (b1 ** 2 <= tot * b2 * (1 + 1e-12)).all()
    # ... and the normalised fields are the raw ones over the photons per column, as the radiance is: the ratios agree
    has = res["intensity"] > 0
    ratio = res["radiancePathLength"].astype(np.float64)[has] / res["intensity"].astype(np.float64)[has]
    assert np.abs(ratio / (b1 / tot)[has] - 1.0).max() <= 3 * 2.0 ** -24
    g.finalize_Integrator()


# ---- 3: launches ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    return cases.step_cloud(ssa=0.95, nlayers=8, ncolumns=8)


TWO = dict(RRI, intensityMus=[1.0, 0.45], intensityPhis=[0.0, 200.0], surfaceAlbedo=0.3)


def test_two_launches_into_one_block_and_zeroing(cloud):
    g = make_gpu(cloud, hg_table(), computeRadiancePathLengths=True, **TWO)
    whole = _run(g, (5, 9), n=20_000)
    seq, sun = M.new_RandomNumberSequence((5, 9)), (0.5, 25.0)
    g.launch(seq, M.new_PhotonStream(sun[0], sun[1], 10_000))
    g.launch(seq, M.new_PhotonStream(sun[0], sun[1], 10_000), zero=False)
    parts = g.finish()
    assert parts["counters"] == whole["counters"] and whole["counters"]["photons"] == 20_000
    assert_same_sums(parts["raw"][:g.layout().counters], whole["raw"][:g.layout().counters], whole["counters"], directions=2, what="old tallies")
    for a, b in zip(_block(g, parts), _block(g, whole)):
        assert (b > 0).all()
        assert_same_sums(a, b, whole["counters"], directions=2, what="radiance path block")
    g._check(g._lib.i3rc_hip_zero_tallies(g._h), "zero")
    assert (g.fetch() == 0).all()
    # a look-ahead call does not look ahead with the kind on: the same launch
    ahead = g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence((5, 9)), M.new_PhotonStream(sun[0], sun[1], 20_000), lookAhead=3)
    assert ahead["counters"] == whole["counters"]
    assert_same_sums(ahead["raw"], whole["raw"], whole["counters"], directions=2, what="compute_batch")
    g.finalize_Integrator()


def test_set_directions_lays_the_block_out_anew(cloud):
    g = make_gpu(cloud, hg_table(), computeRadiancePathLengths=True, **TWO)
    ncol = g.nx * g.ny
    base = lambda nd: 3 * ncol + ncol * g.nz + 2 * nd * ncol + 2 * nd + M.binding.NUM_COUNTERS      # noqa: E731
    assert g.radiance_path_length_layout() == (base(2), base(2) + 2 * ncol, base(2) + 4 * ncol)
    g.specifyParameters(intensityMus=[1.0, 0.7, 0.3], intensityPhis=[0.0, 10.0, 20.0])
    assert g.radiance_path_length_layout() == (base(3), base(3) + 3 * ncol, base(3) + 6 * ncol)
    res = _run(g, (5, 9), n=5_000)
    assert res["radiancePathLength"].shape == (3, g.ny, g.nx) and (res["radiancePathLength"] > 0).all()
    # a caller-bound buffer is refused before anything is touched, as without the kind
    import torch
    buf = torch.zeros(g.layout().total, dtype=torch.float64, device="cuda")
    g._check(g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), buf.numel() * 8), "bind")
    with pytest.raises(M.I3RCError, match="a caller-bound tally buffer is in use; unbind it"):
        g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_radiance_path_lengths: a caller-bound tally buffer is in use"):
        g.specifyParameters(computeRadiancePathLengths=False)
    assert g.radiance_path_length_layout() == (base(3), base(3) + 3 * ncol, base(3) + 6 * ncol)
    g._check(g._lib.i3rc_hip_bind_tally_buffer(g._h, None, 0), "unbind")
    g.specifyParameters(computeRadiancePathLengths=False)
    assert g.radiance_path_length_layout() == (-1, -1, base(3)) and g.layout().total == base(3)
    g.finalize_Integrator()


def test_refusals(cloud):
    seq = lambda: M.new_RandomNumberSequence((5, 9))        # noqa: E731
    sun = lambda n=1000: M.new_PhotonStream(0.5, 25.0, n)   # noqa: E731
    who = "radiance path lengths"
    # no direction
    g = make_gpu(cloud, hg_table(), surfaceAlbedo=0.3, computeRadiancePathLengths=True)
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_launch_batch: {who} are tallied by radiance launches only; no radiance direction is set"):
        g.computeRadiativeTransfer(seq(), sun())
    # a direction that does not point upwards
    g.specifyParameters(intensityMus=[1.0, -0.5], intensityPhis=[0.0, 0.0])
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_launch_batch: {who} need upward radiance directions; direction 2 has uz <= 0"):
        g.computeRadiativeTransfer(seq(), sun())
    g.specifyParameters(**TWO)
    # max cross-section, the contribution limit
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_launch_batch: {who} need ray tracing; max cross-section is in use"):
        g.computeRadiativeTransfer(seq(), sun())
    g.specifyParameters(useRayTracing=True, limitIntensityContributions=True, maxIntensityContribution=0.5)
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_launch_batch: {who} cannot follow limited contributions; the redistributed excess has no path"):
        g.computeRadiativeTransfer(seq(), sun())
    g.specifyParameters(limitIntensityContributions=False)
    # the loops: fused, announced, the three moments calls -- no batch statistics yet
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_run_batches: {who} have no batch statistics yet"):
        g.computeRadiativeTransferBatches((5, 9), 3, 0.5, 25.0, 1000)
    s, accepted = M.host._directional(0.5, 25.0), C.c_int(-1)
    assert g._lib.i3rc_hip_expect_batches(g._h, 5, 9, 4, 1000, C.byref(s), C.byref(accepted)) != 0
    text = g._lib.i3rc_hip_last_error(g._h).decode()
    assert f"i3rc_hip_expect_batches: {who} have no batch statistics yet and are tallied by plain launches only; fused or announced batches cannot give them" in text, text
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_run_batches_moments: {who} have no batch statistics yet"):
        g.computeRadiativeTransferBatchMoments((5, 9), 3, 0.5, 25.0, 1000)
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_get_diagnostic_moments_layout: {who} have no batch statistics yet"):
        g.computeRadiativeTransferDiagnosticMoments((5, 9), 3, 0.5, 25.0, 1000)
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_get_path_moments_layout: {who} have no batch statistics yet"):
        g.computeRadiativeTransferPathMoments((5, 9), 3, 0.5, 25.0, 1000)
    lay = M.binding.MomentsLayout()
    g._check(g._lib.i3rc_hip_get_moments_layout(g._h, C.byref(lay)), "layout")
    bufs = [np.zeros(lay.total) for _ in range(2)] + [np.zeros(M.binding.NUM_COUNTERS)] + [np.zeros(8) for _ in range(2)]
    for call in ("i3rc_hip_run_batches_diagnostic_moments", "i3rc_hip_run_batches_path_moments"):
        assert getattr(g._lib, call)(g._h, 5, 9, 3, 1000, C.byref(s), *[b.ctypes.data_as(M.binding.dp) for b in bufs]) != 0
        text = g._lib.i3rc_hip_last_error(g._h).decode()
        assert f"{call}: {who} have no batch statistics yet" in text, text
    # the replay entry point
    n = 10
    arrays = [np.full(n, f32(0.5)) for _ in range(3)] + [np.full(n, f32(-0.5)), np.zeros(n, np.float32)]
    with pytest.raises(M.I3RCError, match=f"i3rc_hip_run_replay: {who} are tallied by the production stream's kernels only"):
        g.run_replay(M.PhotonStream(arrays=arrays), np.full(1000, f32(0.5)), np.arange(n, dtype=np.int64) * 100)
    # the kinds exclude one another, both ways, in the one sentence
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_path_lengths: radiance path lengths are switched on and their block lies where the path lengths' would; switch them off first"):
        g.specifyParameters(computePathLengths=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_level_fluxes: radiance path lengths are switched on"):
        g.specifyParameters(computeLevelFluxes=True)
    g.specifyParameters(computeRadiancePathLengths=False)
    g.specifyParameters(computePathLengths=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_radiance_path_lengths: path lengths are switched on and their block lies where the radiance path lengths' would; switch them off first"):
        g.specifyParameters(computeRadiancePathLengths=True)
    # ... and the flux path tally's own refusal with directions set stays word for word
    with pytest.raises(M.I3RCError, match=r"i3rc_hip_launch_batch: path lengths are tallied by flux launches only; radiance directions are set \(nDir > 0\)"):
        g.computeRadiativeTransfer(seq(), sun())
    g.specifyParameters(computePathLengths=False)
    # results that were not computed are not reported
    g.computeRadiativeTransfer(seq(), sun())
    with pytest.raises(M.I3RCError, match="reportResults: radiance path length information not available"):
        g.reportResults(radiancePathLength=True)
    g.specifyParameters(computeRadiancePathLengths=True)
    g.computeRadiativeTransfer(seq(), sun())
    out = g.reportResults(radiancePathLength=True, radiancePathLengthSquared=True)
    assert out["radiancePathLength"].shape == out["intensity"].shape == out["radiancePathLengthSquared"].shape == (2, g.ny, g.nx)
    g.finalize_Integrator()


# ---- 4: the shell ---------------------------------------------------------------------------------------------------------------------
def test_shell_radiance_path_lengths_equal_the_python_mirror():
    from tests.test_fortran_shell import BUILD, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "radiancePathTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "radiancePathTest done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("unavailable  T reportResults: radiance path length information not available") for l in lines), r.stdout
    assert any(l.startswith("exclusive    T specifyParameters: i3rc_hip_set_path_lengths: radiance path lengths are switched on") for l in lines), r.stdout
    assert any(l.startswith("wrongshape   T reportResults: radiancePathLengthSquared array is the wrong size") for l in lines), r.stdout
    assert any(l.startswith("offagain     T") for l in lines), r.stdout
    nx, ny, nz, nd = 4, 2, 6, 2
    ext = np.full((nz, ny, nx), f32(0.0002), np.float32)
    for k in range(2, 5):
        for j in range(ny):
            for i in range(nx):
                ext[k, j, i] = f32(0.004) * f32(1 + (i + 1 + j + 1) % 3)
    d = dict(xe=f32(500.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(500.0) * np.arange(ny + 1, dtype=np.float32),
             ze=np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0, 1000.0], np.float32), ext=ext, ssa=np.full_like(ext, f32(0.95)),
             pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, intensityMus=[1.0, 0.6], intensityPhis=[0.0, 100.0],
                 computeRadiancePathLengths=True, **RRI)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((7, 3)), M.new_PhotonStream(0.5, 30.0, 20_000))
    rep = g.reportResults(radiancePathLength=True, radiancePathLengthSquared=True)
    assert res["counters"]["photons"] == 20_000
    for tag, key in (("intensity", "intensity"), ("radPath1", "radiancePathLength"), ("radPath2", "radiancePathLengthSquared")):
        rows = [l.split() for l in lines if l.startswith(tag + " ")]
        assert len(rows) == nd and all(len(row) == 2 + nx * ny for row in rows), rows
        shell = np.array([[float(v) for v in row[2:]] for row in sorted(rows, key=lambda row: int(row[1]))]).reshape(nd, ny, nx)
        assert (rep[key] > 0).all()
        assert np.abs(shell / rep[key].astype(np.float64) - 1.0).max() <= 0.6e-8, (key, shell, rep[key])     # (nine digits are printed: the same float32)
    mean = sorted([l.split() for l in lines if l.startswith("meanPath ")], key=lambda row: int(row[1]))
    assert len(mean) == nd and all(len(row) == 4 for row in mean), mean
    inten = rep["intensity"].astype(np.float64)
    want = [[rep[k].astype(np.float64)[dd].sum() / inten[dd].sum() for k in M.host.RADIANCE_PATH_NAMES] for dd in range(nd)]
    assert all(1000.0 < w[0] and w[0] ** 2 < w[1] for w in want), want                                # (the domain is 1000 m deep: metres, metres squared)
    got = np.array([[float(v) for v in row[2:]] for row in mean])
    assert np.abs(got / np.array(want) - 1.0).max() <= 0.6e-12, (mean, want)                          # (thirteen digits)
    g.finalize_Integrator()


# ---- 5: multiple scattering against the solver's derivative in an absorber ---------------------------------------------------------------
SLAB_G, SLAB_MU0, SLAB_H = 0.85, 0.5, 250.0
SLAB_MUS, SLAB_PHIS = [1.0, 0.5], [0.0, 90.0]
SLAB_CASES = [(1.0, 1.0, 0.0), (1.0, 0.9, 0.5), (10.0, 1.0, 0.5), (0.1, 1.0, 0.5)]


@functools.lru_cache(maxsize=None)
def solver_path_moments(tau, omega, albedo, n=32):
    """(I(0), -dI/d(kH), d2I/d(kH)2 at 0, and the two derivatives' solver terms) per view direction: central differences of the
    adding-doubling solver at tau' = tau + kH, omega' = omega tau / tau' for kH = 1e-3 and 2e-3, their Richardson value, and
    |Richardson - value at 1e-3|"""
    def radiance(h):
        t = tau + h
        return np.array(solve(t, omega * tau / t, SLAB_G, SLAB_MU0, albedo=albedo, radiance_mus=SLAB_MUS, radiance_dphis_deg=SLAB_PHIS, n=n)["intensity"])
    i0 = radiance(0.0)
    d1, d2 = {}, {}
    for h in (1e-3, 2e-3):
        up, dn = radiance(h), radiance(-h)
        d1[h] = -(up - dn) / (2 * h)
        d2[h] = (up - 2 * i0 + dn) / (h * h)
    r1, r2 = (4 * d1[1e-3] - d1[2e-3]) / 3, (4 * d2[1e-3] - d2[2e-3]) / 3
    return i0, r1, r2, np.abs(r1 - d1[1e-3]), np.abs(r2 - d2[1e-3])


@pytest.mark.parametrize("rri", [False, True], ids=["plain", "roulette"])
@pytest.mark.parametrize("tau,omega,albedo", SLAB_CASES)
def test_slab_path_moments_against_the_solver_s_derivative(tau, omega, albedo, rri):
    """I(k) = I(0) <exp(-k L)> for a uniform gas absorber of coefficient k: -dI/dk at 0 is radiancePath1 and d2I/dk2 is radiancePath2
    (domain means, normalised)."""
    i0, r1, r2, s1, s2 = solver_path_moments(tau, omega, albedo)
    d = cases.plane_parallel(optical_depth=tau, ssa=omega, nx=2, ny=2, nlayers=8, thickness=SLAB_H)
    g = make_gpu(d, hg_table(SLAB_G, 299), surfaceAlbedo=albedo, intensityMus=SLAB_MUS, intensityPhis=SLAB_PHIS, computeRadiancePathLengths=True,
                 **(RRI if rri else {}))
    nb, n = 16, (500_000 if tau < 5 else 150_000)
    rows = []
    for b in range(nb):
        r = g.computeRadiativeTransfer(M.new_RandomNumberSequence((911, 1 + b)), M.new_PhotonStream(SLAB_MU0, 0.0, n))
        rows.append(np.concatenate([r[k].astype(np.float64).mean(axis=(1, 2)) for k in ("intensity", "radiancePathLength", "radiancePathLengthSquared")]))
    assert "PhiloxRadiancePathStream" in g.kernel_name()
    rows = np.array(rows)
    mean, se = rows.mean(0), rows.std(0, ddof=1) / np.sqrt(nb)
    want = np.concatenate([i0, r1 * SLAB_H, r2 * SLAB_H ** 2])
    term = np.concatenate([np.zeros(2), s1 * SLAB_H, s2 * SLAB_H ** 2])
    z = (mean - want) / se
    print("tau", tau, "omega", omega, "albedo", albedo, "roulette", rri)
    print("  solver  <L>/H", (r1 / i0).tolist(), "<L^2>/H^2", (r2 / i0).tolist())
    print("  device  <L>/H", (mean[2:4] / mean[0:2] / SLAB_H).tolist(), "<L^2>/H^2", (mean[4:6] / mean[0:2] / SLAB_H ** 2).tolist())
    print("  relative standard errors", (se / np.abs(want)).tolist(), "deviations in standard errors", z.tolist())
    for k in range(2, 6):
        assert abs(mean[k] - want[k]) <= 4 * se[k] + term[k], (k, mean[k], want[k], se[k], term[k])
    g.finalize_Integrator()


# ---- 6: three-dimensional, end to end ------------------------------------------------------------------------------------------------------
def test_the_equivalence_theorem_brackets_a_real_absorber(cloud):
    """1 - x <= exp(-x) <= 1 - x + x^2 / 2: per column and in the domain mean I(0) - k P1 <= I(k) <= I(0) - k P1 + k^2 P2 / 2, I(k) from the
    production ray-queue kernels on the same cloud plus a purely absorbing component of uniform extinction k."""
    from scipy import stats

    conservative = dict(cloud, ssa=np.ones_like(cloud["ssa"]))
    kw = dict(RRI, intensityMus=[1.0, 0.6], intensityPhis=[0.0, 120.0], surfaceAlbedo=0.4)
    sun, nb, n = (0.6, 35.0), 16, 40_000
    g = make_gpu(conservative, hg_table(), computeRadiancePathLengths=True, **kw)
    on = [_run(g, (321, 1 + b), n=n, sun=sun) for b in range(nb)]
    assert "PhiloxRadiancePathStream" in g.kernel_name()
    g.finalize_Integrator()
    i0 = np.array([r["intensity"].astype(np.float64) for r in on])
    p1 = np.array([r["radiancePathLength"].astype(np.float64) for r in on])
    p2 = np.array([r["radiancePathLengthSquared"].astype(np.float64) for r in on])
    # k from the nadir radiance's own mean path: k <L> ~ 0.1
    k = float(f32(0.1 * i0[:, 0].mean() / p1[:, 0].mean()))
    gas = np.full_like(cloud["ext"], f32(k))
    absorbing = dict(conservative, ext=[conservative["ext"], gas], ssa=[conservative["ssa"], np.zeros_like(gas)], pf=[conservative["pf"], conservative["pf"]])
    q = make_gpu(absorbing, [hg_table(), hg_table(0.0, 8)], **kw)
    off = [_run(q, (654, 1 + b), n=n, sun=sun) for b in range(nb)]
    assert "PhiloxStream, true, false" in q.kernel_name(), q.kernel_name()
    q.finalize_Integrator()
    ik = np.array([r["intensity"].astype(np.float64) for r in off])
    lower, upper = i0 - k * p1, i0 - k * p1 + 0.5 * k * k * p2                       # per batch: the bounds' own batch scatter
    mean = lambda a, ax=(0,): a.mean(axis=ax)                                         # noqa: E731
    se = lambda a: a.std(axis=0, ddof=1) / np.sqrt(a.shape[0])                        # noqa: E731
    # domain means, per direction
    dl, du, dk = lower.mean(axis=(2, 3)), upper.mean(axis=(2, 3)), ik.mean(axis=(2, 3))
    width = (du.mean(0) - dl.mean(0)) / dk.mean(0)
    print("k", k, "k <L>", (k * p1.mean(axis=(0, 2, 3)) / i0.mean(axis=(0, 2, 3))).tolist(), "bracket / I", width.tolist())
    assert ((width > 0.001) & (width < 0.05)).all(), width                           # (the test resolves something, and x stays small)
    for d in range(2):
        s_lo, s_up = np.hypot(se(dl)[d], se(dk)[d]), np.hypot(se(du)[d], se(dk)[d])
        print("direction", d, "I(k)", dk.mean(0)[d], "bracket", dl.mean(0)[d], du.mean(0)[d], "combined standard errors", s_lo, s_up,
              "I(0)", i0.mean(axis=(0, 2, 3))[d])
        assert dk.mean(0)[d] >= dl.mean(0)[d] - 4 * s_lo, (d, dk.mean(0)[d], dl.mean(0)[d], s_lo)
        assert dk.mean(0)[d] <= du.mean(0)[d] + 4 * s_up, (d, dk.mean(0)[d], du.mean(0)[d], s_up)
        # the absorber takes something at all: I(k) lies clearly below I(0)
        assert dk.mean(0)[d] < i0.mean(axis=(0, 2, 3))[d] - 4 * np.hypot(se(i0.mean(axis=(2, 3)))[d], se(dk)[d])
    # per column: the excursion allowance of tests.test_gpu_parity._assert_3sigma, against the nearer bound
    below = (mean(lower) - mean(ik)) / np.sqrt(se(lower) ** 2 + se(ik) ** 2)
    above = (mean(ik) - mean(upper)) / np.sqrt(se(upper) ** 2 + se(ik) ** 2)
    z = np.maximum(np.maximum(below, above), 0.0)
    dof = 2 * nb - 2
    expected = 2 * stats.t.sf(3.0, dof) * z.size
    allowed = int(np.ceil(expected + 3 * np.sqrt(expected) + 1))
    zmax = stats.t.isf(1e-3 / (2 * z.size), dof)
    print("per column: largest excursion", z.max(), "of", zmax, "; beyond 3:", int((z > 3).sum()), "of", allowed, "allowed")
    assert (z > 3.0).sum() <= allowed and z.max() < zmax, (z.max(), zmax, int((z > 3).sum()), allowed)
