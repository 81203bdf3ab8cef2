"""Direction cosines of exactly zero in the specialised kernels' voxel step (trace_step_lazy, csrc/tracer.hpp): the quotient of such
an axis is NaN and falls out of the step's minimum; only 0 < |cosine| < 1e-20 still takes the guarded division (Ray::slow).

1. the tracer hook (trace_rays_kernel: the step under test) against the CPU oracle, bit for bit, on rays whose directions have one
   or two zeros of either sign, tiny cosines, and starts on cell faces and edges;
2. a wave that mixes zero and tiny cosines: the guarded path must still serve the tiny ones;
3. whole launches against the general kernels, whose step keeps the guarded division in a branch of its own: flux kernels with
   `==` on every counter and tally word, the one-direction and ring radiance kernels as the kernel-matrix tests compare them."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tools import cases
from tests.sums import assert_same_sums
from tests.test_gpu_parity import hg_table, make_gpu, make_oracle
from tests.test_gpu_start_store import _equal

pytestmark = pytest.mark.gpu
f32 = np.float32
PZ, NZ = f32(0.0), f32(-0.0)
TINIES = (f32(1e-25), f32(-3e-30), f32(1e-39))
SLOW = f32(1e-20)


def _step_cut():
    return cases.step_cloud(ncolumns=4, nlayers=4)


def _unit(rng, n):
    mu = (2 * rng.random(n) - 1).astype(f32)
    phi = (2 * np.pi * rng.random(n)).astype(f32)
    st = np.sqrt(1 - mu * mu, dtype=f32)
    return np.stack([st * np.cos(phi), st * np.sin(phi), mu], axis=1).astype(f32)


def _directions(rng):
    """about 2000 directions; every row has a zero or a tiny cosine"""
    out = []
    for axis in range(3):                                   # along an axis, the other two +0 / -0 in every combination
        for s in (f32(1.0), f32(-1.0)):
            for za in (PZ, NZ):
                for zb in (PZ, NZ):
                    v = [za, zb]
                    v.insert(axis, s)
                    out += [v] * 30
    one = _unit(rng, 550)                                   # phi = 0 (and its mirror image): dy = +-0
    one[:, 0] = np.sqrt(1 - one[:, 2] * one[:, 2], dtype=f32) * np.where(rng.random(550) < 0.5, f32(1), f32(-1))
    one[:, 1] = np.where(rng.random(550) < 0.5, PZ, NZ)
    out += one.tolist()
    hor = _unit(rng, 450)                                   # horizontal: dz = +-0
    phi = (2 * np.pi * rng.random(450)).astype(f32)
    hor[:, 0], hor[:, 1], hor[:, 2] = np.cos(phi), np.sin(phi), np.where(rng.random(450) < 0.5, PZ, NZ)
    out += hor.tolist()
    for t in TINIES:                                        # the tiny classes on each axis, alone and beside a zero
        for axis in range(3):
            v = _unit(rng, 30)
            v[:, axis] = t
            v[15:, (axis + 1) % 3] = np.where(rng.random(15) < 0.5, PZ, NZ)
            out += v.tolist()
    d = np.array(out, f32)
    assert 1900 <= len(d) <= 2100 and ((d == 0).any(axis=1) | ((np.abs(d) < SLOW) & (d != 0)).any(axis=1)).all()
    return d


def _rays(rng, d, dirs, every_horizontal_ray_ends):
    """starts inside cells, a quarter of them exactly on a face or an edge of their cell; a finite optical depth for every ray"""
    n = len(dirs)
    nz, ny, nx = d["ext"].shape
    live = np.abs(dirs) >= SLOW                               # (below that a face is out of every trace's reach)
    ix, iy, iz = rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n)
    if not every_horizontal_ray_ends:
        # Rays that cannot leave through the top or the bottom end only by their optical depth.  They get a layer in which every
        # row and every column holds an extinguishing cell (rays along x or y) and some row or column is nothing else (rays across
        # both), whichever cells a start on a face makes their own.
        e = d["ext"] > 0
        good = [k + 1 for k in range(nz) if e[k].any(axis=1).all() and e[k].any(axis=0).all() and (e[k].all(axis=1).any() or e[k].all(axis=0).any())]
        assert len(good) >= 3, good
        iz = np.where(live[:, 2], iz, rng.choice(good, n))
    idx = np.stack([ix, iy, iz], axis=1).astype(np.int32)
    edges = (d["xe"], d["ye"], d["ze"])
    u = rng.random((n, 3)).astype(f32)
    pos = np.stack([edges[a][idx[:, a] - 1] + u[:, a] * (edges[a][idx[:, a]] - edges[a][idx[:, a] - 1]) for a in range(3)], axis=1).astype(f32)
    on = rng.random(n) < 0.25                                  # a face, or (a third of them) an edge: the lower or the upper one
    for a, chosen in enumerate((rng.random(n) < 0.45, rng.random(n) < 0.45, rng.random(n) < 0.45)):
        pick = on & chosen
        if not every_horizontal_ray_ends:
            pick &= live[:, 2] | (a != 2)                      # (a horizontal ray on a z face would take the next layer for its own)
        upper = rng.random(n) < 0.5
        pos[:, a] = np.where(pick, edges[a][idx[:, a] - 1 + upper], pos[:, a])
    target = (0.02 + 3.0 * rng.random(n)).astype(f32)
    return pos, idx, target


def _compare(g, o, dirs, pos, idx, target):
    tau, p2, i2, steps = g.trace_rays(dirs, pos, idx, target)
    nerr = 0
    for k in range(len(dirs)):
        t, pp, ii, ss = o.trace(dirs[k], pos[k], idx[k], float(target[k]))
        assert f32(t) == tau[k], (k, dirs[k], pos[k], idx[k], t, tau[k])
        assert np.array_equal(pp, p2[k]) and list(i2[k]) == ii and ss == steps[k], (k, dirs[k], pos[k], idx[k], pp, p2[k], ii, i2[k], ss, steps[k])
        nerr += t < 0
    return nerr, tau


@pytest.mark.parametrize("case,place", [("irregular", "auto"), ("irregular", "linear"), ("step cut", "auto"), ("step cut", "linear"),
                                        ("step cut", "columns")])
def test_tracer_bit_exact_with_zero_and_tiny_cosines(oracle, case, place):
    rng = np.random.default_rng(1912)
    tab = hg_table()
    d = _step_cut() if case == "step cut" else cases.irregular_domain()
    assert d["ext"].shape == ((4, 1, 4) if case == "step cut" else (9, 5, 7))
    g = make_gpu(d, tab)
    if place != "auto":
        g.select_grid_place(place)
    o = make_oracle(oracle, d, [tab.inverse_table(9001)])
    dirs = _directions(rng)
    pos, idx, target = _rays(rng, d, dirs, every_horizontal_ray_ends=case == "step cut")
    nerr, tau = _compare(g, o, dirs, pos, idx, target)
    # (a start on the face a ray moves away from... is fine; on the face it moves TOWARDS the first step is 0: the tracer's error)
    assert nerr < len(dirs) // 8, nerr
    assert (tau == target).sum() > len(dirs) // 4              # traces that arrived at their optical depth
    g.finalize_Integrator()


def test_a_wave_that_mixes_tiny_and_zero_cosines(oracle):
    """64 consecutive rays, (0, 0, -1) and (1e-25, 0, -1) in turn: one wave, whose guarded path is entered for the tiny cosines and
    replaces the NaN quotients of the zeros beside them by huge -- and a second wave of zeros alone, which never enters it."""
    rng = np.random.default_rng(64)
    tab = hg_table()
    for d in (_step_cut(), cases.irregular_domain()):
        g = make_gpu(d, tab)
        o = make_oracle(oracle, d, [tab.inverse_table(9001)])
        dirs = np.zeros((128, 3), f32)
        dirs[:, 2] = f32(-1.0)
        dirs[1:64:2, 0] = f32(1e-25)
        dirs[65::4, 1] = NZ
        pos, idx, target = _rays(rng, d, dirs, every_horizontal_ray_ends=True)
        target[::3] = f32(50.0)                                # (some leave through the bottom)
        nerr, tau = _compare(g, o, dirs, pos, idx, target)
        assert nerr < 32 and (tau[1:64:2] >= 0).sum() > 16, (nerr, tau[:64])
        g.finalize_Integrator()


def _launch(g, sun, n):
    g.launch(M.new_RandomNumberSequence((31, 7)), M.new_PhotonStream(*sun, n), firstPhoton=0)
    return g.finish()


@pytest.mark.parametrize("sun", [(1.0, 0.0), (0.5, 0.0)], ids=["mu0 = 1", "mu0 = 0.5, phi = 0"])
@pytest.mark.parametrize("place", ["auto", "linear", "columns"])
def test_flux_kernels_equal_the_general_kernel(sun, place):
    """2e5 photons on the step cut (conservative, black surface: every tallied weight is 1 and the float64 sums are whole numbers): a sun
    at the zenith starts every photon with dx = dy = 0, one at phi = 0 with dy = 0."""
    n = 200_000
    g = make_gpu(_step_cut(), M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]), surfaceAlbedo=0.0)
    g.select_grid_place(place)
    g.set_tuning(kernel="auto")
    got = _launch(g, sun, n)
    name = g.kernel_name()
    assert name.startswith("photon_kernel<PhiloxStream, false, false, GRID_"), name
    g.set_tuning(kernel="general")
    ref = _launch(g, sun, n)
    assert g.kernel_name().startswith("photon_kernel<PhiloxStream, false, true, GRID_"), g.kernel_name()
    c = _equal(g, got, ref, n, ("step cut", name, sun))
    assert c["scatterings"] > n and c["dropped"] < n // 1000, c
    g.finalize_Integrator()


@pytest.mark.parametrize("kernel", ["auto", "ring"])
def test_nadir_radiance_kernels_equal_the_general_kernel(kernel):
    """Nadir radiance on the column clouds: every local-estimate ray has dx = dy = 0.  The one-direction kernel and the ring kernel
    against the general kernel on the same photons: counters identical, tallies equal to the order of their float64 additions."""
    n = 30_001
    params = dict(intensityMus=[1.0], intensityPhis=[0.0], useRussianRouletteForIntensity=True, zetaMin=0.3, surfaceAlbedo=0.2)
    g = make_gpu(cases.column_clouds(), hg_table(), **params)
    g.set_tuning(kernel=kernel)
    got = g.computeRadiativeTransfer(M.new_RandomNumberSequence((17, 5)), M.new_PhotonStream(1.0, 0.0, n))
    name = g.kernel_name()
    assert name.startswith("photon_kernel<PhiloxStream, true, false, GRID_") and ("one direction" in name) == (kernel == "auto"), name
    g.set_tuning(kernel="general")
    ref = g.computeRadiativeTransfer(M.new_RandomNumberSequence((17, 5)), M.new_PhotonStream(1.0, 0.0, n))
    assert g.kernel_name().startswith("photon_kernel<PhiloxStream, true, true, GRID_"), g.kernel_name()
    assert got["counters"] == ref["counters"] and got["counters"]["photons"] == n, (got["counters"], ref["counters"])
    assert got["counters"]["shadowSteps"] > n
    assert_same_sums(got["raw"], ref["raw"], got["counters"], directions=1, what=(name, "general"))
    g.finalize_Integrator()
