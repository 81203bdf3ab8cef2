"""Upward and downward flux at INTERIOR levels of a homogeneous slab over a Lambertian surface: an adding solver in float64 numpy,
the companion of tests/plane_parallel_solver.py (which gives the fluxes at the top and at the surface only).  It traces no photon and
shares nothing with the kernels or the oracle; of plane_parallel_solver it imports the Gauss nodes and the normalised associated
Legendre functions, the rest is written out here.

Method (van de Hulst's adding, as in Hansen & Travis 1974, section 4).  Fluxes need the azimuthal mean only (Fourier mode 0).  For
a wanted level at optical depth t below the top, the part ABOVE it (optical depth t) and the part BELOW it (optical depth tau - t)
are each built by doubling from a layer so thin that single scattering describes it; the part below gets the Lambertian surface
added underneath; the two parts are then added and the radiance field AT THE INTERFACE is kept:
    u = (1 - R_below R_above)^-1 (R_below d_above + E_above s_below)        upward, diffuse
    d = d_above + R_above u                                                 downward, diffuse
with R the reflection operators (quadrature weights inside), d_above the diffuse light the upper part sends down under the beam,
s_below what the lower part (surface included) sends up under a beam of unit strength at ITS top, and E_above = exp(-t / mu0) the
beam's attenuation.  Flux up = 2 pi sum w mu u; flux down = the direct beam E_above + 2 pi sum w mu d -- every arrival, reflected
light coming down again included, as the tallies count it.

Normalisation as plane_parallel_solver's: unit flux through a horizontal plane at the top."""
import numpy as np

from tests.plane_parallel_solver import _gauss_half, _norm_assoc_legendre


def _phase_matrices(beta, mus, mu0):
    lmax = beta.size - 1
    Yp, Ym, Y0 = _norm_assoc_legendre(lmax, 0, mus), _norm_assoc_legendre(lmax, 0, -mus), _norm_assoc_legendre(lmax, 0, np.array([-mu0]))
    b = beta[:, None]
    return (Yp * b).T @ Yp, (Yp * b).T @ Ym, ((Yp * b).T @ Y0)[:, 0], ((Ym * b).T @ Y0)[:, 0]


def _slab(tau, omega, P, mus, w, mu0):
    """(R, T, sUp, sDn, E) of a homogeneous layer of optical depth tau under a beam of flux 1 through its top: doubling from a layer
    of optical depth below 2e-7 (the rule of plane_parallel_solver.solve, so that a whole slab comes out as it does there)."""
    N = mus.size
    if tau <= 0.0:
        return np.zeros((N, N)), np.eye(N), np.zeros(N), np.zeros(N), 1.0
    pSame, pOpp, pSunUp, pSunDn = P
    F0 = 1.0 / mu0
    K = max(0, int(np.ceil(np.log2(tau / 2e-7))))
    d0 = tau / 2.0 ** K
    path = -np.expm1(-d0 / mus)
    c = path * omega / 2.0
    R = c[:, None] * pOpp * w[None, :]
    T = np.diag(1.0 - path) + c[:, None] * pSame * w[None, :]
    fac = omega * F0 / (4.0 * np.pi)
    sUp, sDn = path * fac * pSunUp, path * fac * pSunDn
    E = np.exp(-d0 / mu0)
    I = np.eye(N)
    for _ in range(K):
        G = np.linalg.inv(I - R @ R)
        u = G @ (R @ sDn + E * sUp)
        d = sDn + R @ u
        sUp, sDn = sUp + T @ u, E * sDn + T @ d
        R, T = R + T @ G @ R @ T, T @ G @ T
        E = E * E
    return R, T, sUp, sDn, E


def solve_levels(tau_levels, tau, omega, g, mu0, albedo=0.0, n=64, moments=None, chi=None):
    """Fluxes at the levels whose optical depths BELOW THE TOP are tau_levels (0 = the top, tau = the surface) of a homogeneous slab of
    optical depth tau; phase function as plane_parallel_solver.solve takes it (g, moments, chi).  Returns (fluxUp[], fluxDown[])."""
    mu0 = abs(float(mu0))
    lmax = 2 * n - 1
    beta = (2.0 * np.arange(lmax + 1) + 1.0) * float(g) ** np.arange(lmax + 1)
    if moments is not None:
        beta[int(moments) + 1:] = 0.0
    if chi is not None:
        chi = np.asarray(chi, np.float64)[:lmax + 1]
        beta = np.zeros(lmax + 1)
        beta[:chi.size] = (2.0 * np.arange(chi.size) + 1.0) * chi
    mus, w = _gauss_half(n)
    N = mus.size
    P = _phase_matrices(beta, mus, mu0)
    I = np.eye(N)
    Rs = np.tile((2.0 * albedo * mus * w)[None, :], (N, 1))    # the Lambertian surface as a reflecting layer
    sSurf = np.full(N, albedo / np.pi)                          # ... under a beam of unit flux
    ups, downs = [], []
    for t in np.asarray(tau_levels, np.float64):
        t = min(max(float(t), 0.0), float(tau))
        R1, T1, sUp1, sDn1, E1 = _slab(t, omega, P, mus, w, mu0)
        R2, T2, sUp2, sDn2, E2 = _slab(tau - t, omega, P, mus, w, mu0)
        # the part below with the surface underneath, seen from above
        G = np.linalg.inv(I - Rs @ R2)
        uSurf = G @ (Rs @ sDn2 + E2 * sSurf)
        sBelow = sUp2 + T2 @ uSurf
        RBelow = R2 + T2 @ G @ Rs @ T2
        # the interface
        u = np.linalg.solve(I - RBelow @ R1, RBelow @ sDn1 + E1 * sBelow)
        d = sDn1 + R1 @ u
        ups.append(float(2.0 * np.pi * np.sum(w * mus * u)))
        downs.append(float(E1 + 2.0 * np.pi * np.sum(w * mus * d)))
    return np.array(ups), np.array(downs)
