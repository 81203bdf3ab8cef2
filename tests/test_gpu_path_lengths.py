"""Path-length moments of reflected and transmitted light on the device: the block of 4 nx ny float64 words that
photon_kernel<PhiloxPathStream, false, true, GRID> fills -- per column the sums of w L and w L^2 over the photons that fluxUp and
fluxDown count there, L the photon's geometric path since its start -- and its normalised form, pinned by identities against tallies
the project already trusts, by exact sums and by an independent solver.

  same photons     feature on against the general kernel with it off: every counter identical, the old tallies equal to the order of
                   their float64 additions (tests/sums.py), once per place of the extinction field, and with an explicit source inside
  exact            no extinction, a black surface: every photon travels the same path L0, the float64 sum of its float32 steps, so
                   pathDown1 = fluxDown L0 and pathDown2 = fluxDown L0^2 word for word under a zenith sun, and to the float32 rounding
                   of every step under a slant sun that wraps the domain several times
  reflection       the same domain over albedo 1: the path goes on through the reflection
  pieces           against the actinic flux's block, whose sum over the cells is the sum of the same pieces
  multiple scatt.  <L> and <L^2> against the adding-doubling solver through the equivalence theorem
  launches         split batches, accumulation, zeroing; the refusals; the Fortran shell

Tolerances.  Two runs of the same photons: tests/sums.py.  Exact sums: 2^-52 per term of a float64 sum.  A slant path: three float32
roundings of a coordinate per voxel step (test_a_slant_sun_to_the_rounding_of_every_step).  The solver comparison: 4 standard errors of
the batch means plus the reference's own uncertainty, which must stay below a quarter of a standard error."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.extra_tally import N, PLACES, old as _old, run, step_cloud_3d as _step_cloud_3d
from tests.sums import assert_same_sums
from tests.test_gpu_parity import hg_table, make_gpu
from tools import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = (31, 4)
_run = functools.partial(run, seed=SEED)
FIELDS = ("pathUp1", "pathUp2", "pathDown1", "pathDown2")


def _block(g, res):
    """the four raw fields as (ny, nx) views of a result's packed buffer, by name"""
    *offs, total = g.path_length_layout()
    ncol = g.ny * g.nx
    first = g.layout().counters + M.binding.NUM_COUNTERS
    assert offs == [first + k * ncol for k in range(4)] and total == first + 4 * ncol == len(res["raw"]) == g.layout().total, (offs, total, len(res["raw"]))
    return {name: res["raw"][at:at + ncol].reshape(g.ny, g.nx) for name, at in zip(FIELDS, offs)}


def _flux(g, res, which):
    at = getattr(g.layout(), which)
    return res["raw"][at:at + g.ny * g.nx].reshape(g.ny, g.nx)


# ---- 1: the same photons, once per place of the extinction field -------------------------------------------------------------------
@pytest.mark.parametrize("place,domain", PLACES, ids=[p for p, _ in PLACES])
def test_same_photons_as_the_general_kernel(place, domain):
    d, tabs = K.DOMAINS[domain]()
    g = make_gpu(d, tabs, **K.PARAMS["flux"])          # absorbing cells, a reflecting surface, a slant sun (K.SOURCE)
    g.select_grid_place(K.PLACE_KNOB[place])
    g.set_tuning(kernel="general")
    off = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>", g.kernel_name()
    old_total, ncol = g.layout().total, g.nx * g.ny
    assert g.path_length_layout() == (-1, -1, -1, -1, old_total)
    g.specifyParameters(computePathLengths=True)
    on = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxPathStream, false, true, {place}>", g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == N and on["counters"]["scatterings"] > 0, (on["counters"], off["counters"])
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what=("old tallies", place))
    assert g.layout().total == old_total + 4 * ncol
    blk = _block(g, on)
    assert all((blk[k] > 0).all() for k in FIELDS), blk
    for k in M.host.PATH_LENGTH_NAMES:
        assert on[k].shape == (g.ny, g.nx) and on[k].dtype == np.float32 and np.isfinite(on[k]).all() and (on[k] > 0).all(), k
    # Cauchy-Schwarz, word for word: (sum w L)^2 <= (sum w) (sum w L^2), to the rounding of the float64 sums
    for flux, one, two in (("fluxUp", "pathUp1", "pathUp2"), ("fluxDown", "pathDown1", "pathDown2")):
        assert (blk[one] ** 2 <= _flux(g, on, flux) * blk[two] * (1 + 1e-12)).all(), flux
    plan = g.last_plan()
    assert plan["ldsTrackSums"] == 0 and plan["startStoreBytes"] == 0 and plan["tableInLds"] == 0, plan
    g.specifyParameters(computePathLengths=False)                   # ... and off again: the old buffer, the old kernel
    assert g.layout().total == old_total and g.path_length_layout() == (-1, -1, -1, -1, old_total)
    again = _run(g)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>"
    assert again["counters"] == off["counters"] and "pathLengthUp" not in again
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
    g.specifyParameters(computePathLengths=True)
    on = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    assert "PhiloxPathStream" in g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == n
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what="explicit source")
    blk = _block(g, on)
    assert blk["pathUp1"].sum() > 0 and blk["pathDown1"].sum() > 0
    g.finalize_Integrator()


# ---- 2: exact ------------------------------------------------------------------------------------------------------------------------
SLAB_Z = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)                       # 1 x 1 x 4: layer edges at multiples of 0.25
CLOUD_Z = np.array([0.0, 0.25, 0.75, 1.0, 1.5, 2.25, 2.5], np.float32)            # 8 x 4 x 6, likewise


def _clear_domain(shape):
    """no extinction anywhere; narrow columns, so that a slant path wraps the domain several times"""
    (nx, ny, dx), ze = ((1, 1, 0.25), SLAB_Z) if shape == "1x1x4" else ((8, 4, 0.0625), CLOUD_Z)
    cells = (len(ze) - 1, ny, nx)
    return dict(xe=f32(dx) * np.arange(nx + 1, dtype=np.float32), ye=f32(0.25 / ny) * np.arange(ny + 1, dtype=np.float32), ze=ze,
                ext=np.zeros(cells, np.float32), ssa=np.zeros(cells, np.float32), pf=np.zeros(cells, np.int32))


def _start_height(ze):
    """photon_kernel, zStart: fl32(z0 + fl32(fl32(1 - spacing(1)) * fl32(zMax - z0))), spacing(1) = 2^-23"""
    z = f32(ze[0] + f32(f32(f32(1.0) - f32(2.0 ** -23)) * f32(ze[-1] - ze[0])))
    assert ze[-2] < z < ze[-1]
    return z


def _straight_path(ze):
    """L0 under a zenith sun: the float64 sum of the float32 pieces -- the start height minus the top layer's lower edge, then the
    layer depths, top to bottom, in the order the lane adds them"""
    pieces = [f32(_start_height(ze) - ze[-2])] + [f32(ze[k + 1] - ze[k]) for k in range(len(ze) - 3, -1, -1)]
    total = 0.0
    for p in pieces:
        total += float(p)
    return total


@pytest.mark.parametrize("shape", ["1x1x4", "8x4x6"])
def test_straight_down_through_clear_air_is_exact(shape):
    d = _clear_domain(shape)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computePathLengths=True)
    res = _run(g, sun=(1.0, 0.0))
    c = res["counters"]
    nz = len(d["ze"]) - 1
    assert c["photons"] == N and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == N and c["exitsTop"] == 0 and c["cellSteps"] == N * nz, c
    down, blk = _flux(g, res, "fluxDown"), _block(g, res)          # raw: the photons of each column (every weight is 1)
    assert down.sum() == N
    L0 = _straight_path(d["ze"])
    # (each term is 1 x L0 or 1 x L0 x L0, formed in float64; the words are sums of `down` equal terms: 2^-52 per term)
    err1, err2 = np.abs(blk["pathDown1"] - down * L0), np.abs(blk["pathDown2"] - down * (L0 * L0))
    print("L0", repr(L0), "largest error in units of 2^-52 per term", float((err1 / np.maximum(down * L0, 1e-300)).max() * 2.0 ** 52 / max(down.max(), 1)),
          float((err2 / np.maximum(down * L0 * L0, 1e-300)).max() * 2.0 ** 52 / max(down.max(), 1)))
    assert (err1 <= down * 2.0 ** -52 * (down * L0)).all(), (err1.max(), L0)
    assert (err2 <= down * 2.0 ** -52 * (down * L0 * L0)).all(), (err2.max(), L0)
    assert (blk["pathUp1"] == 0).all() and (blk["pathUp2"] == 0).all()
    # normalised: the mean path of every column's transmitted light is L0, to the float32 rounding of the two fields and the quotient
    has = down > 0
    mean = res["pathLengthDown"].astype(np.float64)[has] / res["fluxDown"].astype(np.float64)[has]
    assert np.abs(mean / L0 - 1.0).max() <= 3 * 2.0 ** -24, np.abs(mean / L0 - 1.0).max()
    assert (res["pathLengthUp"] == 0).all() and (res["pathLengthSquaredUp"] == 0).all()
    g.finalize_Integrator()


@pytest.mark.parametrize("shape", ["1x1x4", "8x4x6"])
def test_a_slant_sun_to_the_rounding_of_every_step(shape):
    """mu0 = 0.5: the photons cross the domain's width many times on their way down, and every voxel step is float32 arithmetic.  What
    a step can lose: its length times dz is what the height advances by, up to three float32 roundings of a height -- the
    difference edge - z or the product step x dz, the quotient or the sum z + step dz, and the stored height -- of at most
    2^-24 zMax each (every height lies in [0, zMax]).  The last step ends ON the surface, z0 = 0 exactly, so the steps of a photon add
    up to zStart / mu0 with an error of at most 3 x 2^-24 zMax / mu0 per step: over the run, the step counter times that."""
    d = _clear_domain(shape)
    mu0 = 0.5
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computePathLengths=True)
    res = _run(g, sun=(mu0, 30.0))
    c = res["counters"]
    nz, z_max = len(d["ze"]) - 1, float(d["ze"][-1])
    assert c["photons"] == N and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == N and c["exitsTop"] == 0, c
    width = float(d["xe"][-1] - d["xe"][0])
    assert z_max * np.sqrt(1 - mu0 ** 2) / mu0 * np.cos(np.deg2rad(30.0)) > 3 * width and c["cellSteps"] > 3 * N * nz       # several domain widths
    down, blk = _flux(g, res, "fluxDown"), _block(g, res)
    assert down.sum() == N and (blk["pathUp1"] == 0).all() and (blk["pathUp2"] == 0).all()
    L = float(_start_height(d["ze"])) / mu0
    per_step = 3 * 2.0 ** -24 * z_max / mu0
    bound1 = (c["cellSteps"] + N) * per_step                        # (+ N: a photon whose last step ends within 2 spacing() of the surface, not on it)
    err1 = abs(blk["pathDown1"].sum() - N * L)
    # (L_i^2 - L^2 = (L_i - L)(L_i + L), and L_i <= L + the photon's own share of the bound)
    bound2 = bound1 * (2 * L + bound1 / N * (c["cellSteps"] / N + 1))
    err2 = abs(blk["pathDown2"].sum() - N * L * L)
    print("steps per photon", c["cellSteps"] / N, "error of the sum / bound", err1 / bound1, err2 / bound2)
    assert err1 <= bound1 and err2 <= bound2, (err1, bound1, err2, bound2)
    g.finalize_Integrator()


# ---- 3: cumulative through a reflection ----------------------------------------------------------------------------------------------
def test_the_path_goes_on_through_a_reflection():
    """The empty domain over albedo 1: every photon arrives at the surface once, with the path L0, is reflected with its weight 1 and
    leaves through the top after another (zMax - surface) / mu >= zMax - spacing(z0) > L0 (the start lies 2^-23 zMax below the top):
    pathUp1 > 2 L0 fluxUp in every column that has any, equality impossible.  There is no closed form to hold the mean against:
    the upward leg is 1 / mu of the depth under a Lambertian law, whose variance is infinite."""
    d = _clear_domain("8x4x6")
    g = make_gpu(d, hg_table(), surfaceAlbedo=1.0, computePathLengths=True)
    n = 20_000
    res = _run(g, n=n, sun=(1.0, 0.0))
    c = res["counters"]
    assert c["photons"] == n and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == n and c["exitsTop"] == n, c
    up, down, blk = _flux(g, res, "fluxUp"), _flux(g, res, "fluxDown"), _block(g, res)
    assert up.sum() == n and down.sum() == n
    L0 = _straight_path(d["ze"])
    assert (np.abs(blk["pathDown1"] - down * L0) <= down * 2.0 ** -52 * (down * L0)).all()
    assert (np.abs(blk["pathDown2"] - down * (L0 * L0)) <= down * 2.0 ** -52 * (down * L0 * L0)).all()
    has = up > 0
    assert has.sum() > 16 and (blk["pathUp1"][has] > 2 * L0 * up[has]).all(), (blk["pathUp1"] - 2 * L0 * up)[has].min()
    assert (blk["pathUp1"][~has] == 0).all() and (blk["pathUp2"][~has] == 0).all()
    assert (blk["pathUp1"] - L0 * up).sum() > L0 * n                    # the upward legs alone are longer than the downward ones
    assert (blk["pathUp2"][has] > (2 * L0) ** 2 * up[has]).all()
    g.finalize_Integrator()


# ---- 4: against the actinic flux, piece for piece --------------------------------------------------------------------------------------
def test_the_paths_are_the_pieces_the_actinic_flux_tallies():
    """Conservative scattering over a black surface, no roulette: every photon carries w = 1 and ends exactly once, through the top or
    on the surface, unless the tracer drops it -- and none is dropped with this seed.  The sum over the cells of the actinic flux's
    raw block (w x length of every piece) is then the sum over the photons of their paths: sum(pathUp1 + pathDown1)."""
    d, mu0 = _step_cloud_3d(1.0), 0.2
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.0, computeActinicFlux=True)
    tracks = _run(g, sun=(mu0, 20.0))
    off, total = g.actinic_flux_layout()
    track_sum = tracks["raw"][off:total].sum()
    g.specifyParameters(computeActinicFlux=False)
    g.specifyParameters(computePathLengths=True)
    paths = _run(g, sun=(mu0, 20.0))
    c = paths["counters"]
    assert c == tracks["counters"] and c["dropped"] == 0 and c["photons"] == N and c["roulette"] == 0, c
    assert c["surfaceHits"] + c["exitsTop"] == N and c["scatterings"] > N
    blk = _block(g, paths)
    assert _flux(g, paths, "fluxUp").sum() + _flux(g, paths, "fluxDown").sum() == N
    path_sum = blk["pathUp1"].sum() + blk["pathDown1"].sum()
    # (either sum adds up one float64 term per voxel step and per arrival, in its own grouping: tests/sums.py with the steps counted)
    tc = dict(c, photons=c["photons"] + c["cellSteps"])
    print("sum of the pieces", track_sum, "sum of the paths", path_sum, "relative difference", abs(track_sum - path_sum) / track_sum)
    assert path_sum > 2 * N * 250.0                                      # (a slant sun at mu0 = 0.2 over 250 m: five times that before any scattering)
    assert_same_sums(np.array([path_sum]), np.array([track_sum]), tc, what="paths against pieces")
    g.finalize_Integrator()


# ---- 5: multiple scattering against the independent solver ---------------------------------------------------------------------------
def _romberg(values, ratio):
    """Richardson's table of estimates at steps h, h / 2, h / 4, ... whose error is a series in powers of h (ratio 2: one-sided
    differences) or of h^2 (ratio 4: central ones); returns (the finest extrapolation, its difference from the one a step coarser)"""
    T = [list(values)]
    for k in range(1, len(values)):
        T.append([(ratio ** k * T[k - 1][i + 1] - T[k - 1][i]) / (ratio ** k - 1) for i in range(len(T[k - 1]) - 1)])
    return T[-1][0], abs(T[-1][0] - T[-2][-1])


@functools.lru_cache(maxsize=None)
def _solver_moments(tau, omega, albedo):
    """(<L> / H, <L^2> / H^2) of (the reflected, the transmitted) light and the reference's own uncertainty of each, from the
    adding-doubling solver by the equivalence theorem: a pure absorber of optical depth t added to the slab turns it into
    solve(tau + t, omega tau / (tau + t)), and F(t) = F(0) <exp(-t L / H)>, so <L> / H = -d ln F / dt and <L^2> / H^2 = F'' / F at t = 0.
    omega < 1: central differences at t = +-0.01 and +-0.005 (a negative t takes absorber away), extrapolated once; the uncertainty is
    the difference between the two step sizes.  omega = 1 has no absorber to take away: one-sided differences, which converge only
    linearly, at t = 0.04 ... 0.0025, Richardson-extrapolated; the uncertainty is the difference between the two finest extrapolations."""
    from tests.plane_parallel_solver import solve
    from tests.test_plane_parallel import G, MU0, _sampled_moments

    def F(t):
        r = solve(tau + t, omega * tau / (tau + t), G, MU0, albedo=albedo, chi=_sampled_moments())
        return np.array([r["fluxUp"], r["fluxDown"]])
    f0 = F(0.0)
    if omega < 1.0:
        first, second = [], []
        for h in (0.01, 0.005):
            fp, fm = F(h), F(-h)
            first.append(-(np.log(fp) - np.log(fm)) / (2 * h))
            second.append((fp - 2 * f0 + fm) / (h * h) / f0)
        (m1, _), (m2, _) = _romberg(first, 4), _romberg(second, 4)
        return m1, m2, np.abs(first[1] - first[0]), np.abs(second[1] - second[0])
    first, second = [], []
    for h in (0.04, 0.02, 0.01, 0.005, 0.0025):
        f1, f2 = F(h), F(2 * h)
        first.append(-(np.log(f1) - np.log(f0)) / h)
        second.append((f0 - 2 * f1 + f2) / (h * h) / f0)
    (m1, u1), (m2, u2) = _romberg(first, 2), _romberg(second, 2)
    return m1, m2, u1, u2


@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("omega,albedo", [(0.9, 0.5), (1.0, 0.0)])
def test_mean_paths_against_the_adding_solver(tau, omega, albedo):
    from tests.test_plane_parallel import G, MOMENTS, MU0, SIGMAS

    nb, n, H = 20, 100_000, 1.0
    ext = np.full((4, 1, 1), f32(tau / H), np.float32)
    d = dict(xe=np.array([0.0, 4.0], np.float32), ye=np.array([0.0, 4.0], np.float32), ze=SLAB_Z * f32(H), ext=ext,
             ssa=np.full_like(ext, f32(omega)), pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, computePathLengths=True)
    per = []
    for b in range(1, nb + 1):
        res = _run(g, n=n, seed=(12, b), sun=(MU0, 0.0))
        blk = _block(g, res)
        up, down = _flux(g, res, "fluxUp").sum(), _flux(g, res, "fluxDown").sum()
        per.append([blk["pathUp1"].sum() / up / H, blk["pathDown1"].sum() / down / H, blk["pathUp2"].sum() / up / H ** 2, blk["pathDown2"].sum() / down / H ** 2])
    per = np.array(per)
    mean, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(nb)
    m1, m2, u1, u2 = _solver_moments(tau, omega, albedo)
    want, unc = np.concatenate([m1, m2]), np.concatenate([u1, u2])
    for k, name in enumerate(("<L> up", "<L> down", "<L^2> up", "<L^2> down")):
        print(f"tau {tau} omega {omega} albedo {albedo} {name}: {mean[k]:.6f} +- {se[k]:.6f}, solver {want[k]:.6f} +- {unc[k]:.2e}, "
              f"difference / tolerance {abs(mean[k] - want[k]) / (SIGMAS * se[k] + unc[k]):.3f}")
    assert (se > 0).all() and (want[:2] > 0.5).all()
    assert (unc < 0.25 * se).all(), ("the reference is not sharp enough for this run", unc, se)
    assert (np.abs(mean - want) <= SIGMAS * se + unc).all(), (tau, omega, albedo, mean - want, se, unc)
    g.finalize_Integrator()


# ---- 6: launches -----------------------------------------------------------------------------------------------------------------------
def test_split_batches_accumulation_and_zeroing():
    d = cases.step_cloud(ssa=0.97, nlayers=16, ncolumns=32)
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computePathLengths=True)
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
    assert all((_block(g, both)[k] > _block(g, whole)[k]).all() for k in FIELDS)
    g.set_lds_tallies(False)                                    # every old sum straight to global memory: the same additions in another order
    plain = _run(g)
    assert g.last_plan()["ldsTallies"] == 0 and "PhiloxPathStream" in g.kernel_name(), g.last_plan()
    assert plain["counters"] == whole["counters"]
    assert_same_sums(plain["raw"], whole["raw"], whole["counters"], what="sums in LDS against global atomics")
    g.set_lds_tallies(True)
    g._check(g._lib.i3rc_hip_zero_tallies(g._h), "zero_tallies")
    assert (g.fetch() == 0).all()
    g.finalize_Integrator()


def test_refusals_leave_the_handle_as_it_was():
    import torch

    d = cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)
    fresh = make_gpu(d, hg_table(), surfaceAlbedo=0.3, computePathLengths=True)
    want = _run(fresh)
    fresh.finalize_Integrator()
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3)
    old_total = g.layout().total
    new_total = old_total + 4 * g.nx * g.ny
    buf = torch.zeros(old_total, dtype=torch.float64, device="cuda")
    g.specifyParameters(computePathLengths=True)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) != 0     # the old length: too short now
    assert b"too small" in g._lib.i3rc_hip_last_error(g._h)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: path lengths are tallied by flux launches only; radiance directions are set"):
        g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
        _run(g)
    g.specifyParameters(computeIntensity=False)
    # (from here on every refused call finds tallies in the buffer, and leaves them and the layout as they are)
    first = _run(g)
    layout = g.path_length_layout()
    assert layout[-1] == new_total

    def unchanged():
        assert g.path_length_layout() == layout and g.layout().total == new_total and g.computePathLengths is True
        assert np.array_equal(g.fetch(), first["raw"])

    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: path lengths need ray tracing; max cross-section is in use"):
        g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N), zero=False)
    with pytest.raises(M.I3RCError, match="i3rc_hip_compute_batch: path lengths need ray tracing; max cross-section is in use"):
        g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N))
    g.specifyParameters(useRayTracing=True)
    unchanged()
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches: path lengths are tallied by plain launches only"):
        g.computeRadiativeTransferBatches(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches_moments: path lengths are tallied by plain launches only"):
        g.computeRadiativeTransferBatchMoments(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_get_diagnostic_moments_layout: path lengths have no batch statistics"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    s, accepted = M.binding.Source(), C.c_int(7)
    s.kind, s.solarMu, s.solarAzimuth = 0, K.SOURCE[0], K.SOURCE[1]
    dummy = np.zeros(8 * new_total, np.float64)
    p = dummy.ctypes.data_as(M.binding.dp)
    assert g._lib.i3rc_hip_run_batches_diagnostic_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, p, p) != 0
    assert b"i3rc_hip_run_batches_diagnostic_moments: path lengths have no batch statistics" in g._lib.i3rc_hip_last_error(g._h)
    assert (dummy == 0).all()
    assert g._lib.i3rc_hip_expect_batches(g._h, SEED[0], SEED[1], 4, 1000, C.byref(s), C.byref(accepted)) != 0 and accepted.value == 0
    assert b"i3rc_hip_expect_batches: path lengths are tallied by plain launches only" in g._lib.i3rc_hip_last_error(g._h)
    unchanged()
    # the three blocks behind the counters share their place: none is switched on while another is
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_level_fluxes: path lengths are switched on"):
        g.specifyParameters(computeLevelFluxes=True)
    with pytest.raises(M.I3RCError, match="i3rc_hip_set_actinic_flux: path lengths are switched on"):
        g.specifyParameters(computeActinicFlux=True)
    assert g.level_flux_layout() == (-1, -1, new_total) and g.actinic_flux_layout() == (-1, new_total)
    unchanged()
    rng = np.random.default_rng(3)
    stream = M.PhotonStream(arrays=[rng.random(8), rng.random(8), np.full(8, 0.5), np.full(8, -0.7), np.zeros(8)])
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_replay: path lengths are tallied by the production stream's kernels only; the replay build has no such kernel"):
        g.run_replay(stream, rng.random(4096).astype(np.float32), np.arange(8) * 512)     # (the mirror clears the tallies before it asks)
    assert g.path_length_layout() == layout and g.layout().total == new_total
    # a normal launch afterwards: what a fresh handle gives; through i3rc_hip_compute_batch too (one launch per call, no look-ahead)
    got = _run(g)
    assert got["counters"] == want["counters"]
    assert_same_sums(got["raw"], want["raw"], want["counters"], what="after the refusals")
    for k in range(3):
        ahead = g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*K.SOURCE, N))
        assert "PhiloxPathStream" in g.kernel_name()
    again = _run(g, seed=(SEED[0], SEED[1] + 2))
    assert ahead["counters"] == again["counters"]
    assert_same_sums(ahead["raw"], again["raw"], again["counters"], what="compute_batch")
    g.specifyParameters(computePathLengths=False)
    assert g.layout().total == old_total and g.path_length_layout() == (-1, -1, -1, -1, old_total)
    assert g._lib.i3rc_hip_normalise_path_lengths(g._h, dummy.ctypes.data_as(M.binding.dp), None, None, None, None) != 0
    assert b"i3rc_hip_normalise_path_lengths: path lengths are not switched on" in g._lib.i3rc_hip_last_error(g._h)
    for other, text in (("computeLevelFluxes", "level fluxes are switched on"), ("computeActinicFlux", "the actinic flux is switched on")):
        g.specifyParameters(**{other: True})
        with pytest.raises(M.I3RCError, match="i3rc_hip_set_path_lengths: " + text):
            g.specifyParameters(computePathLengths=True)
        g.specifyParameters(**{other: False})
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) == 0
    assert g._lib.i3rc_hip_set_path_lengths(g._h, 1) != 0 and b"i3rc_hip_set_path_lengths: a caller-bound tally buffer is in use" in g._lib.i3rc_hip_last_error(g._h)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, None, 0) == 0
    with pytest.raises(M.I3RCError, match="path length information not available"):
        _run(g)
        g.reportResults(pathLengthUp=True)
    assert g.layout().total == old_total and g.computePathLengths is False
    last = _run(g)
    assert "PhiloxPathStream" not in g.kernel_name() and last["counters"]["photons"] == N
    g.finalize_Integrator()


# ---- 7: the Fortran shell --------------------------------------------------------------------------------------------------------------
def test_shell_path_lengths_equal_the_python_mirror():
    from tests.test_fortran_shell import BUILD, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "pathLengthTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "pathLengthTest done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("unavailable  T reportResults: path length information not available") for l in lines), r.stdout
    assert any(l.startswith("exclusive    T specifyParameters: i3rc_hip_set_actinic_flux: path lengths are switched on") for l in lines), r.stdout
    assert any(l.startswith("wrongshape   T reportResults: pathLengthSquaredDown array is the wrong size") for l in lines), r.stdout
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
    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, computePathLengths=True)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((7, 3)), M.new_PhotonStream(0.5, 30.0, 50_000))
    rep = g.reportResults(pathLengthUp=True, pathLengthSquaredUp=True, pathLengthDown=True, pathLengthSquaredDown=True)
    assert res["counters"]["photons"] == 50_000
    for tag, key in zip(("pathUp1", "pathUp2", "pathDown1", "pathDown2"), M.host.PATH_LENGTH_NAMES):
        row = [l.split() for l in lines if l.startswith(tag + " ")]
        assert len(row) == 1 and len(row[0]) == 1 + nx * ny, row
        shell = np.array([float(v) for v in row[0][1:]]).reshape(ny, nx)
        assert rep[key].min() > 100.0                                                              # (metres x incident flux)
        assert np.abs(shell / rep[key].astype(np.float64) - 1.0).max() <= 0.6e-8, (key, shell, rep[key])     # (nine digits are printed: the same float32)
    mean = [l.split() for l in lines if l.startswith("meanPath ")]
    assert len(mean) == 1 and len(mean[0]) == 3, mean
    want = [rep[p].astype(np.float64).sum() / rep[f].astype(np.float64).sum() for p, f in (("pathLengthUp", "fluxUp"), ("pathLengthDown", "fluxDown"))]
    assert 1000.0 < want[1] < want[0]                                                              # (the domain is 1000 m deep, the sun at mu0 = 0.5)
    assert np.abs(np.array([float(v) for v in mean[0][1:]]) / np.array(want) - 1.0).max() <= 0.6e-12, (mean, want)      # (thirteen digits)
    g.finalize_Integrator()
