"""The actinic flux by photon track length on the device: the block of nx ny nz float64 words that
photon_kernel<PhiloxTrackStream, false, true, GRID> fills -- per cell the sum of weight x length over all pieces of photon paths
inside it -- and its normalised form actinicFlux (nz, ny, nx), pinned by identities against tallies the project already trusts, by
exact sums, by closed forms and by an independent solver.

  same photons     feature on against the general kernel with it off: every counter identical, the old tallies equal to the order of
                   their float64 additions (tests/sums.py), once per place of the extinction field, and with an explicit source inside
  exact            zenith sun, no extinction: every photon steps straight down, a step's length is one float32 subtraction of two
                   edges, and float64 sums of equal float32 values are exact -- the block bit for bit, with sums in LDS and without
  closed forms     the direct beam through an absorbing slab with clear layers under a slant sun
  pieces           the direct beam through every cell of an absorbing step cloud under a sun that wraps, against a float64 march
                   written here
  absorption       volumeAbsorption - sum_j ext_j (1 - omega_j) actinicFlux = 0 in expectation, cell by cell, with scattering,
                   reflection and the roulette
  multiple scatt.  (1 - omega) sigma dz <actinicFlux> per layer against the net-flux divergence of tests/level_flux_solver.py
  launches         split batches, accumulation, zeroing, sums in LDS against global atomics; the refusals; the Fortran shell

Tolerances.  Two runs of the same photons: tests/sums.py; a word of the track-length block receives at most one addition per voxel
step or scattering of the run, so its order bound counts the voxel steps as well (_track_counters).  Statistical comparisons: the
rule of tests.test_gpu_parity._assert_3sigma per cell, or 4 standard errors of the batch means, the solver comparison with the 3e-5
tests/test_plane_parallel.py allows for what the solver does not model."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.extra_tally import IRREGULAR_Z, N, PLACES, old as _old, run, step_cloud_3d as _step_cloud_3d
from tests.sums import assert_same_sums
from tests.test_gpu_parity import _assert_3sigma, hg_table, make_gpu
from tools import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = (29, 6)
_run = functools.partial(run, seed=SEED)


def _block(g, res):
    """the raw track-length sums as a (nz, ny, nx) view of a result's packed buffer"""
    off, total = g.actinic_flux_layout()
    n = g.nz * g.ny * g.nx
    assert off == g.layout().counters + M.binding.NUM_COUNTERS and total == off + n == len(res["raw"]) == g.layout().total, (off, total, len(res["raw"]))
    return res["raw"][off:off + n].reshape(g.nz, g.ny, g.nx)


def _track_counters(c):
    """tests.sums.order_rtol bounds the additions a word can have received by the run's tally events; a word of the track-length block
    receives one per voxel step in its cell and one per arrival there: the voxel steps are added to the count"""
    return dict(c, photons=c["photons"] + c["cellSteps"])


# ---- 1: the same photons, once per place of the extinction field -------------------------------------------------------------------
@pytest.mark.parametrize("place,domain", PLACES, ids=[p for p, _ in PLACES])
def test_same_photons_as_the_general_kernel(place, domain):
    d, tabs = K.DOMAINS[domain]()
    g = make_gpu(d, tabs, **K.PARAMS["flux"])          # absorbing cells, a reflecting surface, a slant sun (K.SOURCE)
    g.select_grid_place(K.PLACE_KNOB[place])
    g.set_tuning(kernel="general")
    off = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>", g.kernel_name()
    old_total, ncell = g.layout().total, g.nx * g.ny * g.nz
    assert g.actinic_flux_layout() == (-1, old_total)
    g.specifyParameters(computeActinicFlux=True)
    on = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxTrackStream, false, true, {place}>", g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == N and on["counters"]["scatterings"] > 0, (on["counters"], off["counters"])
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what=("old tallies", place))
    assert g.layout().total == old_total + ncell and g.layout().counters + M.binding.NUM_COUNTERS == g.actinic_flux_layout()[0]
    blk = _block(g, on)
    assert (blk > 0).all() and on["actinicFlux"].shape == (g.nz, g.ny, g.nx) and np.isfinite(on["actinicFlux"]).all()
    assert g.last_plan()["ldsTrackSums"] == (1 if place == "GRID_LDS" else 0), g.last_plan()
    g.specifyParameters(computeActinicFlux=False)                   # ... and off again: the old buffer, the old kernel
    assert g.layout().total == old_total and g.actinic_flux_layout() == (-1, old_total)
    again = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>"
    assert again["counters"] == off["counters"] and "actinicFlux" not in again
    assert_same_sums(again["raw"], off["raw"], off["counters"], what=("off again", place))
    g.finalize_Integrator()


def test_same_photons_with_a_source_inside_the_domain():
    """an explicit stream that starts photons at any height, half of them upwards"""
    d, tabs = K.DOMAINS["step_records"]()
    g = make_gpu(d, tabs, surfaceAlbedo=0.3)
    rng = np.random.default_rng(5)
    n = 5_003
    mu = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.2, 1.0, n)
    arrays = [rng.random(n), rng.random(n), rng.uniform(0.02, 0.98, n), mu, rng.uniform(0, 2 * np.pi, n)]
    g.set_tuning(kernel="general")
    off = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    g.specifyParameters(computeActinicFlux=True)
    on = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    assert "PhiloxTrackStream" in g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == n
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what="explicit source")
    assert (_block(g, on) > 0).all()
    g.finalize_Integrator()


# ---- 2: exact ------------------------------------------------------------------------------------------------------------------------
def _clear_domain(nx, ny, ze):
    shape = (len(ze) - 1, ny, nx)
    return dict(xe=f32(62.5) * np.arange(nx + 1, dtype=np.float32), ye=f32(125.0) * np.arange(ny + 1, dtype=np.float32),
                ze=np.asarray(ze, np.float32), ext=np.zeros(shape, np.float32), ssa=np.zeros(shape, np.float32), pf=np.zeros(shape, np.int32))


@pytest.mark.parametrize("shape,lds", [("8x4x6", True), ("5x1x5", True), ("5x1x5", False)], ids=["8x4x6", "5x1x5 sums in LDS", "5x1x5 global atomics"])
def test_straight_down_through_clear_air_is_exact(shape, lds):
    """Convention of the start height, as the kernels form it (photon_kernel: zStart): a Directional photon starts at
    fl32(z0 + fl32(fl32(1 - spacing(1)) * fl32(zMax - z0))), spacing(1) = 2^-23, every operation rounded to float32; its first step
    ends on the floor of the top layer and has the length fl32(zStart - ze[nz - 1])."""
    ze = np.array([0.0, 30.1, 80.7, 120.3, 170.9, 210.2, 250.6], np.float32) if shape == "8x4x6" else np.array([0.0, 41.3, 77.7, 150.1, 190.9, 233.3], np.float32)
    nx, ny = (8, 4) if shape == "8x4x6" else (5, 1)
    d = _clear_domain(nx, ny, ze)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeActinicFlux=True)
    g.set_lds_tallies(lds)
    res = _run(g, sun=(1.0, 0.0))
    c = res["counters"]
    assert g.last_plan()["ldsTrackSums"] == (1 if lds else 0) and g.last_plan()["place"] == 0, g.last_plan()
    assert c["photons"] == N and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == N
    nz = len(ze) - 1
    assert c["cellSteps"] == N * nz
    lay = g.layout()
    down = res["raw"][lay.fluxDown:lay.fluxDown + nx * ny].reshape(ny, nx)        # raw: the photons of each column (every weight is 1)
    assert down.sum() == N
    z_start = f32(ze[0] + f32(f32(f32(1.0) - f32(2.0 ** -23)) * f32(ze[nz] - ze[0])))
    assert ze[nz - 1] < z_start < ze[nz]
    lengths = np.array([f32(ze[k + 1] - ze[k]) for k in range(nz - 1)] + [f32(z_start - ze[nz - 1])], np.float64)
    blk = _block(g, res)
    want = lengths[:, None, None] * down[None]
    assert (blk == want).all(), np.argwhere(blk != want)[:10]
    assert blk.sum() == N * lengths.sum()
    # normalised: 1 in clear air under a zenith sun, to the float32 rounding of the field and the photons that each column happened to get
    flux = res["actinicFlux"].astype(np.float64) * (N / (nx * ny)) / np.maximum(down[None], 1)
    # (a float32 length over the float64 depth, the field's own rounding, the product here: 2^-24 each; the top layer lacks
    # zMax - zStart <= (zMax - z0) 2^-23 of its depth)
    short = float(ze[nz] - ze[0]) * 2.0 ** -23 / float(ze[nz] - ze[nz - 1])
    assert np.abs(flux[:nz - 1] - 1.0).max() <= 4 * 2.0 ** -24 and np.abs(flux[nz - 1] - 1.0).max() <= short + 4 * 2.0 ** -24, (flux.min(), flux.max())
    g.finalize_Integrator()


# ---- 3: closed form, no scattering ---------------------------------------------------------------------------------------------------
def test_direct_beam_through_an_absorbing_slab_with_clear_layers():
    mu0, nb, n = 0.5, 16, 20_000
    sigma = np.array([0.004, 0.012, 0.0, 0.02, 0.006, 0.0, 0.01, 0.003], np.float32)     # per layer, bottom to top; two layers are clear
    ext = np.ascontiguousarray(np.broadcast_to(sigma[:, None, None], (8, 2, 2)), np.float32)
    d = dict(xe=f32(250.0) * np.arange(3, dtype=np.float32), ye=f32(250.0) * np.arange(3, dtype=np.float32), ze=IRREGULAR_Z, ext=ext,
             ssa=np.zeros_like(ext), pf=(ext > 0).astype(np.int32))
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeActinicFlux=True)
    got = np.array([_run(g, n=n, seed=(SEED[0], 300 + b), sun=(mu0, 20.0))["actinicFlux"].astype(np.float64).mean(axis=(1, 2)) for b in range(nb)])
    dz = np.diff(IRREGULAR_Z.astype(np.float64))
    s = sigma.astype(np.float64)
    tau_bot = np.concatenate([np.cumsum((s * dz)[::-1])[::-1], [0.0]])        # optical depth above level k (the floor of layer k)
    tau_top, tau_bot = tau_bot[1:], tau_bot[:-1]
    with np.errstate(all="ignore"):
        want = np.where(s > 0, (np.exp(-tau_top / mu0) - np.exp(-tau_bot / mu0)) / (s * dz), np.exp(-tau_top / mu0) / mu0)
    mean, se = got.mean(0), got.std(0, ddof=1) / np.sqrt(nb)
    print("largest |difference| / (4 se)", float((np.abs(mean - want) / (4 * se)).max()), "values", want)
    assert (se > 0).all() and want.min() > 0.01 and want.max() > 1.5
    assert (np.abs(mean - want) <= 4 * se).all(), (mean - want, se)
    g.finalize_Integrator()


# ---- 4: where a piece lands ----------------------------------------------------------------------------------------------------------
def _march(d, mu0, az_deg, sub=96):
    """float64 march of the direct beam: a regular lattice of sub x sub start points per column on the top, each followed down layer
    by layer; inside a layer the path is cut at every cell wall it meets (periodic wrap), and a piece of length l in a cell of
    extinction s entered with the Beer-Lambert weight W adds W (1 - exp(-s l)) / s (W l where s = 0) to the cell and leaves with
    W exp(-s l).  Returns the cell means of the actinic flux: the sums per start point of the column and per unit of layer depth."""
    xe, ye, ze = (np.asarray(d[k], np.float64) for k in ("xe", "ye", "ze"))
    ext = np.asarray(d["ext"], np.float64)
    nz, ny, nx = ext.shape
    dx, dy, Lx, Ly = xe[1] - xe[0], ye[1] - ye[0], xe[-1] - xe[0], ye[-1] - ye[0]
    phi, s = np.deg2rad(az_deg), np.sqrt(1 - mu0 * mu0)
    tx, ty = s * np.cos(phi) / mu0, s * np.sin(phi) / mu0                    # horizontal travel per unit of descent
    fx = (np.arange(sub) + 0.5) / sub
    PX, PY = np.meshgrid((xe[:-1, None] + fx[None, :] * dx).ravel(), (ye[:-1, None] + fx[None, :] * dy).ravel())
    PX, PY = PX.ravel(), PY.ravel()
    W = np.ones_like(PX)
    out = np.zeros((nz, ny * nx))
    for layer in range(nz - 1, -1, -1):
        depth = ze[layer + 1] - ze[layer]
        hx, hy = tx * depth, ty * depth                                      # travel across this layer
        cuts = [np.zeros_like(PX), np.ones_like(PX)]
        for p0, h, step in ((PX, hx, dx), (PY, hy, dy)):
            if abs(h) < 1e-12:
                continue
            first = np.floor(np.minimum(p0, p0 + h) / step)
            for m in range(int(np.ceil(abs(h) / step)) + 2):
                cuts.append(np.clip(((first + m) * step - p0) / h, 0.0, 1.0))
        f = np.sort(np.stack(cuts), axis=0)
        for a, b in zip(f[:-1], f[1:]):                                      # the pieces, in the order the photon meets them
            length = (b - a) * depth / mu0
            mid = 0.5 * (a + b)
            ix = np.floor(np.mod(PX + mid * hx, Lx) / dx).astype(int) % nx
            iy = np.floor(np.mod(PY + mid * hy, Ly) / dy).astype(int) % ny
            sg = ext[layer][iy, ix]
            with np.errstate(all="ignore"):
                piece = np.where(sg > 0, W * (-np.expm1(-sg * length)) / np.where(sg > 0, sg, 1.0), W * length)
            np.add.at(out[layer], iy * nx + ix, piece)
            W = W * np.exp(-sg * length)
        PX, PY = PX + hx, PY + hy
    return (out / (sub * sub * np.diff(ze)[:, None])).reshape(nz, ny, nx)


@pytest.mark.parametrize("azimuth", [0.0, 45.0], ids=["along x", "diagonal"])
def test_where_a_piece_lands(azimuth):
    d, mu0 = _step_cloud_3d(0.0), 0.2     # 250 m of descent carry the beam 1225 m: two and a half domain widths
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeActinicFlux=True)
    runs = [dict(actinicFlux=_run(g, n=40_000, seed=(SEED[0], 200 + b), sun=(mu0, azimuth))["actinicFlux"]) for b in range(8)]
    want = _march(d, mu0, azimuth)
    assert want.min() < 0.05 and want.max() > 2.5 and np.allclose(want[-1], 1.0 / mu0, rtol=1e-6)      # (the pattern is there to be missed)
    # (floor: what the march's midpoint rule leaves -- 96 x 96 start points per column, (1 / 96)^2 / 2 = 5e-5 of a cell mean that is
    # at most 1 / mu0 --; the reference is exact otherwise: two equal "batches")
    _assert_3sigma(runs, [dict(actinicFlux=want), dict(actinicFlux=want)], "actinicFlux", floor=5e-5 / mu0)
    g.finalize_Integrator()


# ---- 5: against the absorption, cell by cell -----------------------------------------------------------------------------------------
def test_absorption_is_the_absorption_coefficient_times_the_actinic_flux():
    cloud = _step_cloud_3d(0.97)
    gas = np.full_like(cloud["ext"], f32(0.002))
    d = dict(cloud, ext=[cloud["ext"], gas], ssa=[cloud["ssa"], np.full_like(gas, f32(0.9))], pf=[cloud["pf"], np.ones(gas.shape, np.int32)])
    g = make_gpu(d, [hg_table(), hg_table(0.0, 8)], surfaceAlbedo=0.3, useRussianRoulette=True, computeActinicFlux=True)
    kappa = sum(e.astype(np.float64) * (1.0 - s.astype(np.float64)) for e, s in zip(d["ext"], d["ssa"]))     # sum_j ext_j (1 - omega_j)
    assert (kappa > 0).all()
    runs = []
    for b in range(24):
        res = _run(g, n=20_000, seed=(SEED[0], 400 + b), sun=(0.6, 40.0))
        assert res["counters"]["roulette"] > 0 and res["counters"]["surfaceHits"] > 0
        runs.append(dict(d=res["volumeAbsorption"].astype(np.float64) - kappa * res["actinicFlux"].astype(np.float64)))
    zero = np.zeros_like(runs[0]["d"])
    _assert_3sigma(runs, [dict(d=zero), dict(d=zero)], "d")
    means = np.array([r["d"].mean() for r in runs])
    se = means.std(ddof=1) / np.sqrt(len(means))
    print("domain mean of d", means.mean(), "standard error", se)
    assert abs(means.mean()) <= 4 * se, (means.mean(), se)
    g.finalize_Integrator()


# ---- 6: multiple scattering against the independent solver ---------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("albedo", [0.0, 0.5])
def test_layer_absorption_against_the_adding_solver(tau, albedo):
    from tests.level_flux_solver import solve_levels
    from tests.test_plane_parallel import G, MOMENTS, MU0, SIGMAS, MODEL, _sampled_moments

    omega, nb, n = 0.9, 16, 50_000
    ze = np.array([0.0, 20.0, 70.0, 95.0, 160.0, 215.0, 250.0], np.float32)                 # six layers of unequal thickness
    ext = np.full((6, 1, 4), f32(tau) / f32(250.0), np.float32)
    d = dict(xe=f32(125.0) * np.arange(5, dtype=np.float32), ye=np.array([0.0, 500.0], np.float32), ze=ze, ext=ext,
             ssa=np.full_like(ext, f32(omega)), pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, computeActinicFlux=True)
    sigma, dz = float(ext[0, 0, 0]), np.diff(ze.astype(np.float64))
    got = np.array([(1.0 - float(f32(omega))) * sigma * dz * _run(g, n=n, seed=(10, b), sun=(MU0, 0.0))["actinicFlux"].astype(np.float64).mean(axis=(1, 2))
                    for b in range(1, nb + 1)])
    depth = sigma * (float(ze[-1]) - ze.astype(np.float64))                                 # optical depth above level k (0: the surface)
    up, down = solve_levels(depth, depth[0], omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    net = down - up
    want = net[1:] - net[:-1]                                                               # what flows into a layer and not out of it
    mean, se = got.mean(0), got.std(0, ddof=1) / np.sqrt(nb)
    print("tau", tau, "albedo", albedo, "largest |difference| / (4 se + 3e-5)", float((np.abs(mean - want) / (SIGMAS * se + MODEL)).max()), "values", want)
    assert (want > 1e-3).all()
    assert (np.abs(mean - want) <= SIGMAS * se + MODEL).all(), (tau, albedo, mean - want, se)
    g.finalize_Integrator()


# ---- 7: launches ---------------------------------------------------------------------------------------------------------------------
def test_split_batches_accumulation_zeroing_and_lds_sums():
    d = cases.step_cloud(ssa=0.97, nlayers=16, ncolumns=32)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computeActinicFlux=True)
    whole = _run(g)
    assert g.last_plan()["ldsTrackSums"] == 1 and g.last_plan()["ldsGrid"] == 1, g.last_plan()
    tc = _track_counters(whole["counters"])
    n1, n2 = 12_345, 9_000
    seq = M.new_RandomNumberSequence(SEED)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, n1), firstPhoton=0, zero=True)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, n2), firstPhoton=n1, zero=False)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, N - n1 - n2), firstPhoton=n1 + n2, zero=False)
    parts = g.finish()
    assert parts["counters"] == whole["counters"]
    assert_same_sums(parts["raw"], whole["raw"], tc, what="one launch against three")
    other = _run(g, seed=(SEED[0], SEED[1] + 1))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N), zero=True)
    g.launch(M.new_RandomNumberSequence((SEED[0], SEED[1] + 1)), M.new_PhotonStream(*K.SOURCE, N), zero=False)
    both = g.finish()
    total = {k: whole["counters"][k] + other["counters"][k] for k in whole["counters"]}
    assert both["counters"] == total
    assert_same_sums(both["raw"], whole["raw"] + other["raw"], _track_counters(total), what="a second batch adds")
    assert (_block(g, both) > _block(g, whole)).all()
    g.set_lds_tallies(False)                                    # every sum straight to global memory: the same additions in another order
    plain = _run(g)
    assert g.last_plan()["ldsTrackSums"] == 0 and g.last_plan()["ldsTallies"] == 0 and "PhiloxTrackStream" in g.kernel_name(), g.last_plan()
    assert plain["counters"] == whole["counters"]
    assert_same_sums(plain["raw"], whole["raw"], tc, what="sums in LDS against global atomics")
    g.set_lds_tallies(True)
    g._check(g._lib.i3rc_hip_zero_tallies(g._h), "zero_tallies")
    assert (g.fetch() == 0).all()
    g.finalize_Integrator()


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    import torch

    d = cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)
    fresh = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computeActinicFlux=True)
    want = _run(fresh)
    fresh.finalize_Integrator()
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3)
    old_total = g.layout().total
    buf = torch.zeros(old_total, dtype=torch.float64, device="cuda")
    g.specifyParameters(computeActinicFlux=True)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) != 0     # the old length: too short now
    assert b"too small" in g._lib.i3rc_hip_last_error(g._h)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: the actinic flux is tallied by flux launches only; radiance directions are set"):
        g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
        _run(g)
    g.specifyParameters(computeIntensity=False)
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: the actinic flux needs ray tracing; max cross-section is in use"):
        _run(g)
    with pytest.raises(M.I3RCError, match="i3rc_hip_compute_batch: the actinic flux needs ray tracing; max cross-section is in use"):
        g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N))
    g.specifyParameters(useRayTracing=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches: the actinic flux is tallied by plain launches only"):
        g.computeRadiativeTransferBatches(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches_moments: the actinic flux is tallied by plain launches only"):
        g.computeRadiativeTransferBatchMoments(SEED, 3, *K.SOURCE, 1000)
    s, accepted = M.binding.Source(), C.c_int(7)
    s.kind, s.solarMu, s.solarAzimuth = 0, K.SOURCE[0], K.SOURCE[1]
    assert g._lib.i3rc_hip_expect_batches(g._h, SEED[0], SEED[1], 4, 1000, C.byref(s), C.byref(accepted)) != 0 and accepted.value == 0
    assert b"i3rc_hip_expect_batches: the actinic flux is tallied by plain launches only" in g._lib.i3rc_hip_last_error(g._h)
    rng = np.random.default_rng(3)
    stream = M.PhotonStream(arrays=[rng.random(8), rng.random(8), np.full(8, 0.5), np.full(8, -0.7), np.zeros(8)])
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_replay: the actinic flux is tallied by the production stream's kernels only; the replay build has no such kernel"):
        g.run_replay(stream, rng.random(4096).astype(np.float32), np.arange(8) * 512)
    # the two blocks behind the counters share their place: neither is switched on while the other is
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_level_fluxes: the actinic flux is switched on"):
        g.specifyParameters(computeLevelFluxes=True)
    assert g.level_flux_layout() == (-1, -1, old_total + g.nx * g.ny * g.nz)
    # a normal launch afterwards: what a fresh handle gives; through i3rc_hip_compute_batch too (one launch per call, no look-ahead)
    got = _run(g)
    assert got["counters"] == want["counters"]
    assert_same_sums(got["raw"], want["raw"], _track_counters(want["counters"]), what="after the refusals")
    for k in range(3):
        ahead = g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*K.SOURCE, N))
        assert "PhiloxTrackStream" in g.kernel_name()
    again = _run(g, seed=(SEED[0], SEED[1] + 2))
    assert ahead["counters"] == again["counters"]
    assert_same_sums(ahead["raw"], again["raw"], _track_counters(again["counters"]), what="compute_batch")
    g.specifyParameters(computeActinicFlux=False)
    assert g.layout().total == old_total and g.actinic_flux_layout() == (-1, old_total)
    g.specifyParameters(computeLevelFluxes=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_actinic_flux: level fluxes are switched on"):
        g.specifyParameters(computeActinicFlux=True)
    g.specifyParameters(computeLevelFluxes=False)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) == 0
    assert g._lib.i3rc_hip_set_actinic_flux(g._h, 1) != 0 and b"i3rc_hip_set_actinic_flux: a caller-bound tally buffer is in use" in g._lib.i3rc_hip_last_error(g._h)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, None, 0) == 0
    with pytest.raises(M.I3RCError, match="actinic flux information not available"):
        _run(g)
        g.reportResults(actinicFlux=True)
    assert g.layout().total == old_total and g.actinic_flux_layout() == (-1, old_total) and g.computeActinicFlux is False
    last = _run(g)
    assert "PhiloxTrackStream" not in g.kernel_name() and last["counters"]["photons"] == N
    g.finalize_Integrator()


# ---- 9: the Fortran shell ------------------------------------------------------------------------------------------------------------
def test_shell_actinic_flux_equals_the_python_mirrors():
    from tests.test_fortran_shell import BUILD, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "actinicFluxTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "actinicFluxTest done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("unavailable  T reportResults: actinic flux information not available") for l in lines), r.stdout
    assert any(l.startswith("wrongshape   T reportResults: actinicFlux array is the wrong size") for l in lines), r.stdout
    assert any(l.startswith("offagain     T") for l in lines), r.stdout
    nx, ny, nz = 4, 2, 6
    ext = np.full((nz, ny, nx), f32(0.0002), np.float32)
    for k in range(2, 5):
        for j in range(ny):
            for i in range(nx):
                ext[k, j, i] = f32(0.004) * f32(1 + (i + 1 + j + 1) % 3)
    d = dict(xe=f32(500.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(500.0) * np.arange(ny + 1, dtype=np.float32),
             ze=np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0, 1000.0], np.float32), ext=ext, ssa=np.full_like(ext, f32(0.95)),
             pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, computeActinicFlux=True)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((7, 3)), M.new_PhotonStream(0.5, 30.0, 50_000))
    rep = g.reportResults(actinicFlux=True)
    rows = [l.split() for l in lines if l.startswith("actinic ")]
    assert [int(row[1]) for row in rows] == list(range(nz)), rows
    shell = np.array([[float(v) for v in row[2:]] for row in rows]).reshape(nz, ny, nx)
    assert np.abs(shell - rep["actinicFlux"]).max() <= 0.6e-6, np.abs(shell - rep["actinicFlux"]).max()     # (six decimals are printed)
    assert res["counters"]["photons"] == 50_000 and rep["actinicFlux"].min() > 0.5
    g.finalize_Integrator()
