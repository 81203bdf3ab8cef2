"""Level fluxes, the parts that need no GPU: the C ABI's new symbols, the independent solver tests/level_flux_solver.py held to its
own three checks, and the resource figures of the kernels that tally them.

The solver's checks, each to 1e-9:
  1. its top and surface values are plane_parallel_solver.solve's fluxUp and fluxDown (both build a whole slab by the same doubling);
  2. omega = 1: the net flux is the same at every level.  Doubling starts from a single-scattering layer of optical depth d0 <= 2e-7
     (the rule check 1 ties this solver to), whose energy balance is off in second order; over a slab that adds up to about
     tau d0 / mu^2: plane_parallel_solver.solve itself has fluxUp + fluxDown - 1 = 2.3e-8 at tau = 1 (its own test asks 1e-6), and a
     solver that equals it at both ends cannot have a constant net flux there.  The 1e-9 check therefore runs where the REFERENCE'S OWN
     defect is below the bound -- tau = 0.002 (5.4e-10) and 0.0005; at tau = 0.01 it is 2.4e-9 already -- and asserts that it is.
     At tau = 1 and 10, the depths the GPU test uses the solver at, the spread is asserted against a bound from the doubling start:
     a start layer of optical depth d0 takes 1 - exp(-d0 / mu) = d0 / mu - d0^2 / (2 mu^2) + ... out of a stream and hands on what
     first-order single scattering makes of it, so that its energy balance is off by a relative d0 / (2 mu) of what it scatters; all
     the scattering a photon undergoes in the slab passes through such layers, so the net flux carries a defect of the order of
     d0 <= 2e-7 times the flux-weighted mean of 1 / (2 mu), a few tenths of d0 however thick the slab.  THICK_BOUND = 5e-8 is
     d0_max / 4.  Measured: 2.3e-8 (tau = 1) and 2.2e-8 (tau = 10) at both albedos -- interior figures; the reference's end-to-end
     defect is 2.3e-8 at tau = 1 and 4.3e-9 at tau = 10.  A wrong reflection term in the adding step would show at the size of the
     fluxes themselves there;
  3. omega = 0: exp(-tau_k / mu0) comes down at every level; albedo exp(-tau / mu0) goes up at the surface, and above it what is
     left of that isotropic light, albedo exp(-tau / mu0) 2 E3(optical depth below the level) -- compared on the solver's own
     nodes to 1e-9 and with an independent quadrature of E3 to the nodes' accuracy."""
import os
import sys

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests.level_flux_solver import solve_levels
from tests.plane_parallel_solver import _gauss_half, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("i3rc_hip_set_level_fluxes", "i3rc_hip_get_level_flux_layout", "i3rc_hip_normalise_level_fluxes")
G, MU0 = 0.85, 0.5
THICK_BOUND = 5e-8   # (the module's docstring, check 2)


def test_level_flux_symbols_are_exported_and_bound():
    lib = M.binding.load()
    header = open(os.path.join(ROOT, "include", "i3rc_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in M.binding.SYMBOLS, name
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name


@pytest.mark.parametrize("tau,omega,albedo", [(1.0, 1.0, 0.0), (10.0, 0.9, 0.5), (1.0, 0.9, 0.5), (10.0, 1.0, 0.0), (0.1, 1.0, 0.5)])
def test_solver_ends_are_the_plane_parallel_solvers(tau, omega, albedo):
    up, down = solve_levels([0.0, tau], tau, omega, G, MU0, albedo=albedo)
    want = solve(tau, omega, G, MU0, albedo=albedo)
    assert abs(up[0] - want["fluxUp"]) < 1e-9 and abs(down[1] - want["fluxDown"]) < 1e-9, (up, down, want)
    assert abs(down[0] - 1.0) < 1e-9                      # no diffuse light comes down through the top
    assert abs(up[1] - albedo * down[1]) < 1e-9           # a Lambertian surface sends up its albedo of what arrives


@pytest.mark.parametrize("tau", [0.0005, 0.002])
@pytest.mark.parametrize("albedo", [0.0, 0.5])
def test_solver_conserves_the_net_flux(tau, albedo):
    frac = np.array([0.0, 0.08, 0.31, 0.5, 0.77, 0.93, 1.0])
    up, down = solve_levels(frac * tau, tau, 1.0, G, MU0, albedo=albedo)
    net = down - up
    ref = solve(tau, 1.0, G, MU0, albedo=albedo)
    defect = abs(ref["fluxUp"] + (1.0 - albedo) * ref["fluxDown"] - 1.0)
    print("net flux spread", float(np.abs(net - net[0]).max()), "the reference's own energy defect", defect)
    assert defect < 1e-9, defect                          # (where the doubling start's second-order defect is below the bound: see above)
    assert np.abs(net - net[0]).max() < 1e-9, net - net[0]
    assert abs(net[0] - (1.0 - albedo) * down[-1]) < 1e-9


@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("albedo", [0.0, 0.5])
def test_solver_conserves_the_net_flux_of_thick_slabs_to_the_doubling_starts_defect(tau, albedo):
    frac = np.array([0.0, 0.08, 0.31, 0.5, 0.77, 0.93, 1.0])
    up, down = solve_levels(frac * tau, tau, 1.0, G, MU0, albedo=albedo)
    net = down - up
    print("tau", tau, "albedo", albedo, "net flux spread", float(np.abs(net - net[0]).max()))
    assert np.abs(net - net[0]).max() < THICK_BOUND, net - net[0]
    assert abs(net[0] - (1.0 - albedo) * down[-1]) < THICK_BOUND and net[0] > 0.05    # ... and it is the flux the surface keeps


def test_solver_without_scattering():
    tau, albedo = 3.0, 0.4
    levels = np.array([0.0, 0.2, 0.9, 1.7, 2.6, 3.0])
    up, down = solve_levels(levels, tau, 0.0, G, MU0, albedo=albedo)
    assert np.abs(down - np.exp(-levels / MU0)).max() < 1e-9, down - np.exp(-levels / MU0)
    assert abs(up[-1] - albedo * np.exp(-tau / MU0)) < 1e-9
    # above the surface the reflected light is isotropic radiance attenuated along each slant path: 2 E3 of the depth below the level
    mus, w = _gauss_half(64)
    below = tau - levels
    on_nodes = albedo * np.exp(-tau / MU0) * np.array([2.0 * np.sum(w * mus * np.exp(-b / mus)) for b in below])
    assert np.abs(up - on_nodes).max() < 1e-9, up - on_nodes
    x = (np.arange(400000) + 0.5) / 400000                # E3 by a midpoint rule of its own
    e3 = np.array([np.mean(x * np.exp(-b / x)) for b in below])
    assert np.abs(up - albedo * np.exp(-tau / MU0) * 2.0 * e3).max() < 1e-6


def test_level_flux_kernels_keep_their_state_in_registers():
    """as tests/test_build_isa.py asks of the production kernels: no spilled vector register, no scratch"""
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources

    rows = [r for r in resources() if r["name"].startswith("photon_kernel<PhiloxLevelStream")]
    assert sorted(r["name"] for r in rows) == sorted(f"photon_kernel<PhiloxLevelStream, false, true, {p}>" for p in
                                                     ("GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE")), [r["name"] for r in rows]
    for r in rows:
        print(r["name"], "VGPRs", r["VGPRs"], "SGPR spills", r["SGPRs Spill"], "occupancy", r["Occupancy [waves/SIMD]"])
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (r["name"], r["VGPRs Spill"], r["ScratchSize [bytes/lane]"])
