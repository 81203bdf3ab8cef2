"""Level fluxes on the device: levelFluxUp / levelFluxDown [nz + 1][ny][nx] of photon_kernel<PhiloxLevelStream, false, true, GRID>
pinned by identities against tallies the project already trusts, by closed forms and by an independent solver.

  same photons     feature on against the general kernel with it off: every counter identical, the old tallies equal to the order of
                   their float64 additions (tests/sums.py), once per place of the extinction field, and with an explicit source inside
  boundaries       levelFluxDown[0] = fluxDown, levelFluxUp[nz] = fluxUp per column; sum of levelFluxDown[nz] = photons, exactly;
                   levelFluxUp[0] = albedo fluxDown per column to the float32 rounding of each reflected weight
  conservation     net flux into every layer = what the layer absorbs; omega = 1: one net flux at every level
  closed forms     direct beam through an absorbing slab of irregular layers; an empty domain over a reflecting surface
  crossings        the direct beam through every level of every column of an absorbing step cloud under a slant sun that wraps,
                   against a float64 march written here
  multiple scatt.  domain means at every level against tests/level_flux_solver.py
  launches         split batches, accumulation, zeroing; the refusals; the Fortran shell against the Python mirror

Tolerances.  Two runs of the same photons: tests/sums.py.  A reflection makes w' = fl32(w a): |w' - w a| <= 2^-24 w a, so a column's
levelFluxUp[0] is within 2^-24 a fluxDown of a fluxDown (and within surfaceHits 2^-24 a, weights being at most 1 without the roulette).
A scattering makes w' = fl32(w omega) and tallies fl32(w fl32(1 - omega)): without the roulette a layer's balance is off by at most
scatterings 2^-24 (largest weight 1) plus the order term of the float64 sums.  Statistical comparisons: 4 standard errors (binomial, or
of the batch means), the solver comparison with its 3e-5 for what the solver does not model (tests/test_plane_parallel.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.extra_tally import IRREGULAR_Z, N, PLACES, old as _old, run, step_cloud_3d as _step_cloud_3d
from tests.sums import assert_same_sums, order_rtol
from tests.test_gpu_parity import _assert_3sigma, hg_table, make_gpu
from tools import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = (23, 4)
U = 2.0 ** -24      # unit roundoff of float32
# The exact balances hold for any number of photons, and they want a run without a dropped photon (the reference's tracer error, Q4:
# about one in 2.6e6 traces on these domains, counted with the CPU oracle): a few thousand photons, some 2e5 traces
N_EXACT = 6_001
_run = functools.partial(run, seed=SEED)


def _levels(g, res):
    """raw levelFluxUp, levelFluxDown as (nz + 1, ny, nx) views of a result's packed buffer"""
    up, down, total = g.level_flux_layout()
    n = (g.nz + 1) * g.ny * g.nx
    assert up >= 0 and down == up + n and total == down + n == len(res["raw"]), (up, down, total, len(res["raw"]))
    return res["raw"][up:up + n].reshape(g.nz + 1, g.ny, g.nx), res["raw"][down:down + n].reshape(g.nz + 1, g.ny, g.nx)


def _field(g, res, name):
    lay, ncol = g.layout(), g.nx * g.ny
    o = getattr(lay, name)
    return res["raw"][o:o + ncol].reshape(g.ny, g.nx)


def _check_boundaries(g, res):
    up, down = _levels(g, res)
    c = res["counters"]
    assert_same_sums(down[0], _field(g, res, "fluxDown"), c, what="levelFluxDown[0] = fluxDown")
    assert_same_sums(up[g.nz], _field(g, res, "fluxUp"), c, what="levelFluxUp[nz] = fluxUp")


# ---- 4, 5: the same photons, once per place of the extinction field ------------------------------------------------------------------
@pytest.mark.parametrize("place,domain", PLACES, ids=[p for p, _ in PLACES])
def test_same_photons_as_the_general_kernel(place, domain):
    d, tabs = K.DOMAINS[domain]()
    g = make_gpu(d, tabs, **K.PARAMS["flux"])          # absorbing cells, a reflecting surface, a slant sun (K.SOURCE)
    g.select_grid_place(K.PLACE_KNOB[place])
    g.set_tuning(kernel="general")
    off = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>", g.kernel_name()
    old_total = g.layout().total
    assert g.level_flux_layout() == (-1, -1, old_total)
    g.specifyParameters(computeLevelFluxes=True)
    on = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxLevelStream, false, true, {place}>", g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == N and on["counters"]["scatterings"] > 0, (on["counters"], off["counters"])
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what=("old tallies", place))
    assert g.layout().total == old_total + 2 * (g.nz + 1) * g.nx * g.ny and g.layout().counters + M.binding.NUM_COUNTERS == g.level_flux_layout()[0]
    _check_boundaries(g, on)
    up, down = _levels(g, on)
    assert down[g.nz].sum() == on["counters"]["photons"]           # a Directional source: every photon comes in through the top, exactly
    assert (up >= 0).all() and (down >= 0).all() and up[0].sum() > 0
    g.specifyParameters(computeLevelFluxes=False)                   # ... and off again: the old buffer, the old kernel
    assert g.layout().total == old_total
    again = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>"
    assert again["counters"] == off["counters"]
    assert_same_sums(again["raw"], off["raw"], off["counters"], what=("off again", place))
    g.finalize_Integrator()


def test_same_photons_with_a_source_inside_the_domain():
    """an explicit stream that starts photons at any height, half of them upwards.  A photon is counted at the face of its start layer
    that lies behind it: a face belongs to two layers, so a photon that starts downwards in layer a is an outflow of layer a + 1 that
    never flowed in, and one that starts upwards in layer a likewise of layer a - 1 -- the source term of the layers' balance, known
    from the stream's own arrays (roulette off)"""
    d, tabs = K.DOMAINS["step_records"]()
    g = make_gpu(d, tabs, surfaceAlbedo=0.3, useRussianRoulette=False)
    rng = np.random.default_rng(5)
    n = 5_003        # (small on purpose: the tracer drops about one photon in 2.6e6 traces, and the balance wants none dropped)
    mu = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.2, 1.0, n)
    arrays = [rng.random(n), rng.random(n), rng.uniform(0.02, 0.98, n), mu, rng.uniform(0, 2 * np.pi, n)]
    g.set_tuning(kernel="general")
    off = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    g.specifyParameters(computeLevelFluxes=True)
    on = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    assert "PhiloxLevelStream" in g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["dropped"] == 0
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what="explicit source")
    _check_boundaries(g, on)
    ze = np.asarray(d["ze"], np.float32)
    z = ze[0] + arrays[2].astype(np.float32) * (ze[-1] - ze[0])                 # the kernel's own float32 start height
    layer = np.searchsorted(ze, z, side="right")                                # 1-based start layer
    assert layer.min() >= 1 and layer.max() <= g.nz and np.abs(z[:, None] - ze[None, :]).min() > 1e-3    # (no start within rounding of an interface)
    source = np.zeros(g.nz + 2)
    np.add.at(source, layer + np.where(mu < 0, 1, -1), 1.0)                     # the layer on the other side of the face behind the photon
    _check_conservation(g, on, source=source[1:g.nz + 1])
    up, down = _levels(g, on)
    assert down[g.nz].sum() == np.sum((mu < 0) & (layer == g.nz)) and down.reshape(g.nz + 1, -1).sum(axis=1)[g.nz] > 0
    g.finalize_Integrator()


# ---- 5 (reflection), 6: conservation --------------------------------------------------------------------------------------------------
def _absorbed_by_layer(g, res):
    lay, ncell = g.layout(), g.nx * g.ny * g.nz
    return res["raw"][lay.volumeAbsorption:lay.volumeAbsorption + ncell].reshape(g.nz, -1).sum(axis=1)


def _check_conservation(g, res, source=None):
    """roulette off: (down[k] - up[k]) - (down[k-1] - up[k-1]) over the domain = the layer's absorption (less `source`: weight counted
    as leaving the layer that never entered it -- photons started inside the domain)"""
    c = res["counters"]
    assert c["dropped"] == 0, c
    up, down = _levels(g, res)
    U_, D_ = up.reshape(g.nz + 1, -1).sum(axis=1), down.reshape(g.nz + 1, -1).sum(axis=1)
    net = D_ - U_
    got, want = net[1:] - net[:-1], _absorbed_by_layer(g, res) - (0.0 if source is None else source)
    tol = c["scatterings"] * U * 1.0 + order_rtol(c) * (D_[1:] + U_[1:] + D_[:-1] + U_[:-1] + np.abs(want))
    print("conservation: largest defect", float(np.abs(got - want).max()), "bound", float(tol.min()))
    assert (np.abs(got - want) <= tol).all(), (got - want, tol)


@pytest.mark.parametrize("shape", ["16x1x8", "8x4x6"])
def test_conservation_and_reflection_without_the_roulette(shape):
    d = _step_cloud_3d(0.95) if shape == "8x4x6" else cases.step_cloud(ssa=0.95, nlayers=8, ncolumns=16)
    albedo = 0.4
    g = make_gpu(d, hg_table(), surfaceAlbedo=albedo, useRussianRoulette=False, computeLevelFluxes=True)
    res = _run(g, n=N_EXACT, sun=(0.6, 40.0))
    c = res["counters"]
    assert c["roulette"] == 0 and c["surfaceHits"] > 0
    _check_boundaries(g, res)
    _check_conservation(g, res)
    # a reflected photon adds its weight after the reflection, where it was reflected
    up, _ = _levels(g, res)
    a, fdown = float(f32(albedo)), _field(g, res, "fluxDown")
    tol = U * a * fdown + order_rtol(c) * a * fdown
    assert (tol <= c["surfaceHits"] * U * a + 1e-300).all()                      # (the same bound from the surface-hit counter: weights are at most 1)
    print("reflection: largest defect", float(np.abs(up[0] - a * fdown).max()), "bound", float(tol.max()))
    assert (np.abs(up[0] - a * fdown) <= tol).all(), (np.abs(up[0] - a * fdown).max(), tol.max())
    g.finalize_Integrator()


def test_conservative_scattering_has_one_net_flux():
    d = cases.step_cloud(ssa=1.0, nlayers=8, ncolumns=16)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, useRussianRoulette=False, computeLevelFluxes=True)
    res = _run(g, n=N_EXACT)
    c = res["counters"]
    assert c["dropped"] == 0
    up, down = _levels(g, res)
    U_, D_ = up.reshape(g.nz + 1, -1).sum(axis=1), down.reshape(g.nz + 1, -1).sum(axis=1)
    net = D_ - U_
    assert (np.abs(net - net[0]) <= order_rtol(c) * (D_ + U_ + D_[0] + U_[0])).all(), net - net[0]
    assert net[0] > 0 and _absorbed_by_layer(g, res).sum() == 0
    g.finalize_Integrator()


def test_conservation_with_the_roulette_within_the_batch_noise():
    d = cases.step_cloud(ssa=0.9, nlayers=8, ncolumns=16)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, useRussianRoulette=True, computeLevelFluxes=True)
    defects = []
    for b in range(8):
        res = _run(g, n=4_000, seed=(SEED[0], 100 + b))
        assert res["counters"]["dropped"] == 0 and res["counters"]["roulette"] > 0
        up, down = _levels(g, res)
        net = (down - up).reshape(g.nz + 1, -1).sum(axis=1)
        defects.append(((net[1:] - net[:-1]) - _absorbed_by_layer(g, res)) / res["counters"]["photons"])
    defects = np.array(defects)
    mean, se = defects.mean(0), defects.std(0, ddof=1) / np.sqrt(len(defects))
    assert (np.abs(mean) <= 4 * se + 1e-12).all(), (mean, se)
    g.finalize_Integrator()


# ---- 7: closed forms --------------------------------------------------------------------------------------------------------------------
def _slab(tau, ssa, nx=2, ny=2):
    ext = np.full((8, ny, nx), f32(tau) / f32(250.0), np.float32)
    return dict(xe=f32(250.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(250.0) * np.arange(ny + 1, dtype=np.float32), ze=IRREGULAR_Z,
                ext=ext, ssa=np.full_like(ext, f32(ssa)), pf=np.ones(ext.shape, np.int32))


def test_direct_beam_through_an_absorbing_slab():
    tau, mu0, n = 3.0, 0.5, 200_000
    g = make_gpu(_slab(tau, 0.0), hg_table(), surfaceAlbedo=0.0, computeLevelFluxes=True)
    res = _run(g, n=n, sun=(mu0, 0.0))
    up, down = _levels(g, res)
    assert (up == 0).all()
    got = down.reshape(9, -1).sum(axis=1) / n
    depth = float(f32(tau) / f32(250.0)) * (250.0 - IRREGULAR_Z.astype(np.float64))    # optical depth above each level
    want = np.exp(-depth / mu0)
    se = np.sqrt(want * (1 - want) / n)
    assert (np.abs(got - want) <= 4 * se).all(), (got - want, se)                      # (the top level, se = 0, is exact: next line)
    assert got[8] == 1.0
    g.finalize_Integrator()


def test_empty_domain_over_a_reflecting_surface():
    d = _slab(0.0, 0.0)
    d["pf"] = np.zeros_like(d["pf"])
    n, albedo = 50_000, 0.4
    g = make_gpu(d, hg_table(), surfaceAlbedo=albedo, useRussianRoulette=False, computeLevelFluxes=True)
    res = _run(g, n=n, sun=(0.7, 10.0))
    up, down = _levels(g, res)
    assert (down.reshape(9, -1).sum(axis=1) == n).all()
    got = up.reshape(9, -1).sum(axis=1) / n
    assert (np.abs(got - albedo) <= U * albedo * (1 + 1e-6)).all(), got - albedo        # every reflected weight is fl32(0.4)
    g.finalize_Integrator()


# ---- 8: where a crossing lands ----------------------------------------------------------------------------------------------------------
def _direct_beam(d, mu0, az_deg, sub=96):
    """float64 march: the mean transmission from the top to every level over the crossing points of every column.  Crossing points
    are uniform over a level (the entry points are uniform over the top); each column takes sub x sub of them; the path back up
    is cut at every cell wall it meets, layer by layer."""
    xe, ye, ze = (np.asarray(d[k], np.float64) for k in ("xe", "ye", "ze"))
    ext = np.asarray(d["ext"], np.float64)
    nz, ny, nx = ext.shape
    dx, dy, Lx, Ly = xe[1] - xe[0], ye[1] - ye[0], xe[-1] - xe[0], ye[-1] - ye[0]
    phi = np.deg2rad(az_deg)
    s = np.sqrt(1 - mu0 * mu0)
    tx, ty = s * np.cos(phi) / mu0, s * np.sin(phi) / mu0                   # horizontal travel per unit of descent
    fx = (np.arange(sub) + 0.5) / sub
    X = (xe[:-1, None] + fx[None, :] * dx).ravel()                           # (nx * sub)
    Y = (ye[:-1, None] + fx[None, :] * dy).ravel()
    PX, PY = np.meshgrid(X, Y)                                               # crossing points, (ny * sub, nx * sub)
    out = np.zeros((nz + 1, ny, nx))
    for k in range(nz + 1):
        tau = np.zeros_like(PX)
        for layer in range(k, nz):                                           # the layers above level k, from the level upwards
            z0, z1 = ze[layer] - ze[k], ze[layer + 1] - ze[k]                # heights above the level
            x0, y0, hx, hy = PX - tx * z0, PY - ty * z0, -tx * (z1 - z0), -ty * (z1 - z0)   # going UP moves against the sun's travel
            cuts = [np.zeros_like(PX), np.ones_like(PX)]
            for p0, h, step in ((x0, hx, dx), (y0, hy, dy)):
                if abs(h).max() == 0:
                    continue
                first = np.floor(np.minimum(p0, p0 + h) / step)
                for m in range(int(np.ceil(abs(h).max() / step)) + 2):
                    cuts.append(np.clip(((first + m) * step - p0) / h, 0.0, 1.0))
            f = np.sort(np.stack(cuts), axis=0)
            mid, df = 0.5 * (f[1:] + f[:-1]), f[1:] - f[:-1]
            ix = np.floor(np.mod(x0[None] + mid * hx[None], Lx) / dx).astype(int) % nx
            iy = np.floor(np.mod(y0[None] + mid * hy[None], Ly) / dy).astype(int) % ny
            tau += (ext[layer][iy, ix] * df).sum(axis=0) * (z1 - z0) / mu0
        out[k] = np.exp(-tau).reshape(ny, sub, nx, sub).mean(axis=(1, 3))
    return out


@pytest.mark.parametrize("azimuth", [0.0, 45.0], ids=["along x", "diagonal"])
def test_where_a_crossing_lands(azimuth):
    d, mu0 = _step_cloud_3d(0.0), 0.2     # 250 m of descent carry the beam 1225 m: two and a half domain widths
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeLevelFluxes=True)
    runs = []
    for b in range(8):
        res = _run(g, n=40_000, seed=(SEED[0], 200 + b), sun=(mu0, azimuth))
        assert (res["levelFluxUp"] == 0).all()
        runs.append(dict(levelFluxDown=res["levelFluxDown"]))
    want = _direct_beam(d, mu0, azimuth)
    assert want[:-1].min() < 0.05 and want[:-1].max() > 0.5 and np.allclose(want[-1], 1.0)      # (the pattern is there to be missed)
    # (floor: what the march's midpoint rule leaves -- 96 x 96 crossing points per column, (1 / 96)^2 / 2 = 5e-5 of a transmission
    # that is at most 1 --; the reference is exact otherwise: two equal "batches")
    _assert_3sigma(runs, [dict(levelFluxDown=want), dict(levelFluxDown=want)], "levelFluxDown", floor=5e-5)
    g.finalize_Integrator()


def test_where_an_upward_crossing_lands():
    """The columns of UPWARD crossings, photon by photon: an explicit stream of photons that start just above the surface of an empty
    8 x 4 x 6 domain (black surface), each with its own slant direction, fly straight out through the top -- up to six domain widths
    of travel.  Every level's column follows from the start point in float64; photons whose crossing of any level comes within 5 cm
    of a column's wall (the tracer's own float32 walk is good to millimetres here) are left out of the stream, so that the float32
    arithmetic of the kernel cannot decide otherwise:
    the level block must then hold exactly these counts."""
    d = _step_cloud_3d(0.0)
    d["ext"] = np.zeros_like(d["ext"]); d["pf"] = np.zeros_like(d["pf"]); d["ssa"] = np.zeros_like(d["ssa"])
    xe, ye, ze = (np.asarray(d[k], np.float64) for k in ("xe", "ye", "ze"))
    nz, ny, nx = d["ext"].shape
    rng = np.random.default_rng(11)
    n = 6000
    px, py, pz = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32), np.full(n, 0.02, np.float32)   # z = 5 m: in layer 1
    mu, phi = rng.uniform(0.15, 1.0, n).astype(np.float32), rng.uniform(0, 2 * np.pi, n).astype(np.float32)
    x0, y0, z0 = px.astype(np.float64) * xe[-1], py.astype(np.float64) * ye[-1], float(pz[0]) * ze[-1]
    s = np.sqrt(1.0 - mu.astype(np.float64) ** 2)
    cols, keep = [], np.ones(n, bool)
    for k in range(1, nz + 1):                                               # the levels above the start layer's floor
        t = (ze[k] - z0) / mu.astype(np.float64)
        x, y = np.mod(x0 + t * s * np.cos(phi.astype(np.float64)), xe[-1]), np.mod(y0 + t * s * np.sin(phi.astype(np.float64)), ye[-1])
        fx, fy = x / (xe[1] - xe[0]), y / (ye[1] - ye[0])
        keep &= (np.abs(fx - np.round(fx)) * (xe[1] - xe[0]) > 5e-2) & (np.abs(fy - np.round(fy)) * (ye[1] - ye[0]) > 5e-2)
        cols.append((np.floor(fy).astype(int) % ny) * nx + np.floor(fx).astype(int) % nx)
    fx0, fy0 = x0 / (xe[1] - xe[0]), y0 / (ye[1] - ye[0])
    keep &= (np.abs(fx0 - np.round(fx0)) * (xe[1] - xe[0]) > 5e-2) & (np.abs(fy0 - np.round(fy0)) * (ye[1] - ye[0]) > 5e-2)
    cols = [np.floor(fy0).astype(int) * nx + np.floor(fx0).astype(int)] + cols   # level 0: the start column (the face behind the photon)
    assert keep.sum() > 0.95 * n
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeLevelFluxes=True)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=[a[keep] for a in (px, py, pz, mu, phi)]))
    assert res["counters"]["photons"] == keep.sum() and res["counters"]["exitsTop"] + res["counters"]["dropped"] == keep.sum()
    up, down = _levels(g, res)
    assert (down == 0).all()
    if res["counters"]["dropped"] == 0:
        want = np.stack([np.bincount(c[keep], minlength=nx * ny) for c in cols]).reshape(nz + 1, ny, nx)
        assert (up == want).all(), np.argwhere(up != want)[:10]
        assert (want[nz] != want[nz - 1]).any() and (want[1] != want[0]).any()      # (the photons do change columns on the way)
    else:                                                                          # (a dropped photon's segment tallies nothing above its start)
        assert up.reshape(nz + 1, -1).sum(axis=1)[0] == keep.sum()
        pytest.fail("a photon was dropped: choose another seed for this stream")
    g.finalize_Integrator()


# ---- 9: multiple scattering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("omega", [1.0, 0.9])
@pytest.mark.parametrize("albedo", [0.0, 0.5])
def test_slab_level_fluxes_against_the_adding_solver(tau, omega, albedo):
    from tests.level_flux_solver import solve_levels
    from tests.test_plane_parallel import G, MOMENTS, MU0, SIGMAS, MODEL, _sampled_moments

    d = cases.plane_parallel(optical_depth=tau, ssa=omega, nx=2, ny=2, nlayers=8)
    g = make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, computeLevelFluxes=True)
    n, nb = (150_000 if tau < 5 else 60_000), 8
    ups, downs = [], []
    for b in range(1, nb + 1):
        res = _run(g, n=n, seed=(10, b), sun=(MU0, 0.0))
        ups.append(res["levelFluxUp"].astype(np.float64).mean(axis=(1, 2)))
        downs.append(res["levelFluxDown"].astype(np.float64).mean(axis=(1, 2)))
    depth = tau * (1.0 - np.arange(9) / 8.0)                       # optical depth above level k
    want_up, want_down = solve_levels(depth, tau, omega, G, MU0, albedo=albedo, chi=_sampled_moments())
    for name, got, want in (("up", np.array(ups), want_up), ("down", np.array(downs), want_down)):
        mean, se = got.mean(0), got.std(0, ddof=1) / np.sqrt(nb)
        print(name, "largest |difference| / (4 se + 3e-5)", float((np.abs(mean - want) / (SIGMAS * se + MODEL)).max()))
        assert (np.abs(mean - want) <= SIGMAS * se + MODEL).all(), (name, tau, omega, albedo, mean - want, se)
    g.finalize_Integrator()


# ---- 10: split and accumulate ---------------------------------------------------------------------------------------------------------------
def test_split_batches_accumulation_and_zeroing():
    d = cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computeLevelFluxes=True)
    whole = _run(g)
    n1 = 12_345
    seq = M.new_RandomNumberSequence(SEED)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, n1), firstPhoton=0, zero=True)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, N - n1), firstPhoton=n1, zero=False)
    parts = g.finish()
    assert parts["counters"] == whole["counters"]
    assert_same_sums(parts["raw"], whole["raw"], whole["counters"], what="one launch against two")
    other = _run(g, seed=(SEED[0], SEED[1] + 1))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N), zero=True)
    g.launch(M.new_RandomNumberSequence((SEED[0], SEED[1] + 1)), M.new_PhotonStream(*K.SOURCE, N), zero=False)
    both = g.finish()
    total = {k: whole["counters"][k] + other["counters"][k] for k in whole["counters"]}
    assert both["counters"] == total
    assert_same_sums(both["raw"], whole["raw"] + other["raw"], total, what="a second batch adds")
    up, down = _levels(g, both)
    assert up.sum() > 0 and down.sum() > 0
    g._check(g._lib.i3rc_hip_zero_tallies(g._h), "zero_tallies")
    assert (g.fetch() == 0).all()
    g.finalize_Integrator()


# ---- 11: refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    import torch

    d = cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)
    fresh = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computeLevelFluxes=True)
    want = _run(fresh)
    fresh.finalize_Integrator()
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3)
    old_total = g.layout().total
    buf = torch.zeros(old_total, dtype=torch.float64, device="cuda")
    g.specifyParameters(computeLevelFluxes=True)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) != 0     # the old length: too short now
    assert b"too small" in g._lib.i3rc_hip_last_error(g._h)
    with pytest.raises(M.I3RCError, match="radiance directions are set"):
        g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
        _run(g)
    g.specifyParameters(computeIntensity=False)
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match="max cross-section is in use"):
        _run(g)
    with pytest.raises(M.I3RCError, match="max cross-section is in use"):
        g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N))
    g.specifyParameters(useRayTracing=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches: level fluxes are tallied by plain launches only"):
        g.computeRadiativeTransferBatches(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches_moments: level fluxes are tallied by plain launches only"):
        g.computeRadiativeTransferBatchMoments(SEED, 3, *K.SOURCE, 1000)
    s, accepted = M.binding.Source(), C.c_int(7)
    s.kind, s.solarMu, s.solarAzimuth = 0, K.SOURCE[0], K.SOURCE[1]
    assert g._lib.i3rc_hip_expect_batches(g._h, SEED[0], SEED[1], 4, 1000, C.byref(s), C.byref(accepted)) != 0 and accepted.value == 0
    assert b"i3rc_hip_expect_batches: level fluxes are tallied by plain launches only" in g._lib.i3rc_hip_last_error(g._h)
    # a normal launch afterwards: what a fresh handle gives; through i3rc_hip_compute_batch too (one launch per call, no look-ahead)
    got = _run(g)
    assert got["counters"] == want["counters"]
    assert_same_sums(got["raw"], want["raw"], want["counters"], what="after the refusals")
    for k in range(3):
        ahead = g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*K.SOURCE, N))
        assert "PhiloxLevelStream" in g.kernel_name()
    again = _run(g, seed=(SEED[0], SEED[1] + 2))
    assert ahead["counters"] == again["counters"]
    assert_same_sums(ahead["raw"], again["raw"], again["counters"], what="compute_batch")
    g.specifyParameters(computeLevelFluxes=False)
    assert g.layout().total == old_total and g.level_flux_layout() == (-1, -1, old_total)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) == 0
    assert g._lib.i3rc_hip_set_level_fluxes(g._h, 1) != 0 and b"caller-bound" in g._lib.i3rc_hip_last_error(g._h)    # (a bound buffer: unbind first)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, None, 0) == 0
    with pytest.raises(M.I3RCError, match="level fluxes weren't computed"):
        _run(g)
        g.reportResults(levelFluxUp=True)
    g.finalize_Integrator()


# ---- 12: the Fortran shell ----------------------------------------------------------------------------------------------------------------
def test_shell_level_fluxes_equal_the_python_mirrors():
    from tests.test_fortran_shell import BUILD, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "levelFluxTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "level flux test done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("unavailable  T reportResults: level flux information not available") for l in lines), r.stdout
    assert any(l.startswith("wrongshape   T reportResults: levelFluxUp array is the wrong size") for l in lines), r.stdout
    assert any(l.startswith("offagain     T") for l in lines), r.stdout
    for key in ("copied", "copyrun"):      # copy_Integrator with the feature on: the original's results, and the same batch again
        row = [l.split() for l in lines if l.startswith(key + " ")]
        assert len(row) == 1 and row[0][1] == "F" and float(row[0][2]) == 0.0 and float(row[0][3]) == 0.0, (key, row)
    nx, ny, nz = 4, 2, 6
    ext = np.full((nz, ny, nx), f32(0.0002), np.float32)
    for k in range(2, 5):
        for j in range(ny):
            for i in range(nx):
                ext[k, j, i] = f32(0.004) * f32(1 + (i + 1 + j + 1) % 3)
    d = dict(xe=f32(500.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(500.0) * np.arange(ny + 1, dtype=np.float32),
             ze=np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0, 1000.0], np.float32), ext=ext, ssa=np.full_like(ext, f32(0.95)),
             pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, computeLevelFluxes=True)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((7, 3)), M.new_PhotonStream(0.5, 30.0, 50_000))
    rep = g.reportResults(levelFluxUp=True, levelFluxDown=True)
    for key, name in (("levelup", "levelFluxUp"), ("leveldown", "levelFluxDown")):
        rows = [l.split() for l in lines if l.startswith(key + " ")]
        assert [int(row[1]) for row in rows] == list(range(nz + 1)), rows
        shell = np.array([[float(v) for v in row[2:]] for row in rows]).reshape(nz + 1, ny, nx)
        assert np.abs(shell - rep[name]).max() <= 0.6e-6, (name, np.abs(shell - rep[name]).max())     # (six decimals are printed)
    assert res["counters"]["photons"] == 50_000
    g.finalize_Integrator()
