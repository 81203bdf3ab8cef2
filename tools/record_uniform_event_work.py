"""The cases of tests/test_gpu_uniform_event_work.py, and the recorder of their work counters.

The specialised flux kernels of plain launches (photon_kernel, STORE) wrap a photon that crosses a side wall of the periodic domain one
axis at a time, decide absorption, the cell index and the roulette block from one word of launch facts (DevProblem::eventFlags) and make
the inverse table's reciprocal length once per wave.  What they count is pinned to what the commit BEFORE that change counted: run
there, once, on a GPU,
  python3 tools/record_uniform_event_work.py            -> tests/golden/uniform_event_work_parent.json
(I3RC_LIB=other.so: another build of the library, e.g. that commit's) writes the eleven counters (binding.COUNTER_NAMES) of every case,
after checking that all six kernels and the general kernel agree on them.  The test imports CASES, integrator() and run() from here, so
that the recorded launches and the tested ones are the same; the kernels, their knobs and run() are those of
tools/record_event_bookkeeping.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import i3rc_monte_carlo_model_amd as M   # noqa: E402
from tools import record_event_bookkeeping as R   # noqa: E402

if os.environ.get("I3RC_LIB"):
    M.build.LIB = os.path.abspath(os.environ["I3RC_LIB"]); M.build.needs_build = lambda: False

f32 = np.float32
SEED = (31, 7)
GOLDEN = os.path.join(ROOT, "tests", "golden", "uniform_event_work_parent.json")
KERNELS, KNOB = R.KERNELS, R.KNOB

# The event phase's variants: single-scattering albedo, surface albedo, Russian roulette.
#   one / one-rr     nothing absorbs over a black surface: no weight ever leaves 1 (kWeightStaysOne), with the roulette asked for and not
#   absorb / -rr     omega = 0.9: the absorption region and, with roulette, plays and photons that lose
#   lambert          albedo 0.3: weights fall at the surface only, reflections go on
#   faint            albedo 1e-30 (above tiny: not a black surface): a reflected photon carries 1e-30, and its second reflection ends it
PHYSICS = {
    "one": dict(ssa=1.0, albedo=0.0, roulette=False),
    "one-rr": dict(ssa=1.0, albedo=0.0, roulette=True),
    "absorb": dict(ssa=0.9, albedo=0.0, roulette=False),
    "absorb-rr": dict(ssa=0.9, albedo=0.0, roulette=True),
    "lambert": dict(ssa=1.0, albedo=0.3, roulette=False),
    "faint": dict(ssa=1.0, albedo=1e-30, roulette=False),
}
AZIMUTHS = (40.0, 130.0, 220.0, 310.0)   # one per quadrant: x and y walls in both directions, cx and cy of equal and of opposite sign
MU0 = 0.35

# name: domain, photons, omega, albedo, roulette, (mu0, phi)
CASES = {}
for _dom in ("2x1x2", "3x2x4"):
    for _phi in AZIMUTHS:
        for _name, _p in PHYSICS.items():
            CASES[f"{_dom} phi={_phi:.0f} {_name}"] = dict(domain=_dom, photons=4097, sun=(MU0, _phi), **_p)
CASES["step16"] = dict(domain="step16", photons=20001, ssa=1.0, albedo=0.0, roulette=True, sun=(1.0, 0.0))   # (the benchmark's own launch)


def domain(which, ssa):
    """2 x 1 x 2 and 3 x 2 x 4 cells whose widths are a fraction of a free path (0.25 wide, extinction 1 ... 3: 0.25 ... 0.75 free paths),
    under a slant sun: most voxel steps end on an x or y face, and in a domain two or three cells wide -- one in y -- half of those
    faces, or all of them, are side walls.  Optical depth 0.7 ... 2.1 per column: a photon scatters some ten times, so that the weights
    of the absorbing and reflecting cases stay above 2^-16 (tests/test_gpu_event_bookkeeping.py: the sums are exact)"""
    if which == "step16":
        from tools import cases

        return cases.step_cloud(ssa=ssa, nlayers=16), 64
    nx, ny, nz = (2, 1, 2) if which == "2x1x2" else (3, 2, 4)
    ze = np.array([0.0, 0.3, 1.0], f32) if nz == 2 else np.array([0.0, 0.3, 0.45, 0.8, 1.0], f32)
    ext = np.zeros((nz, ny, nx), f32)
    ext[1:] = (f32(1.0) + f32(0.4) * np.arange(nx * ny, dtype=f32).reshape(ny, nx))[None]
    d = dict(xe=(f32(0.25) * np.arange(nx + 1)).astype(f32), ye=(f32(0.25) * np.arange(ny + 1)).astype(f32), ze=ze, ext=ext,
             ssa=np.full(ext.shape, f32(ssa)), pf=np.ones(ext.shape, np.int32))
    return d, 32


def integrator(case):
    c = CASES[case]
    d, moments = domain(c["domain"], c["ssa"])
    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    dom.addOpticalComponent("cloud", d["ext"], d["ssa"], d["pf"], M.PhaseFunctionTable([M.henyey_greenstein(0.85, moments)]))
    g = M.new_Integrator(dom)
    g.specifyParameters(surfaceAlbedo=c["albedo"], useRussianRoulette=c["roulette"])
    return g


def run(g, case, place, tbl, general=False):
    """one launch of the case on one of the six kernels, or on the general kernel at the same place of the field"""
    c = CASES[case]
    g.select_grid_place(KNOB[place])
    g.set_tuning(kernel="general" if general else ("auto" if tbl else "lane"))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*c["sun"], c["photons"]), firstPhoton=0)
    res = g.finish()
    assert g.kernel_name() == R.kernel_name(place, tbl and not general, general), g.kernel_name()
    return res


def main():
    out = {}
    for case in CASES:
        g = integrator(case)
        seen = [run(g, case, place, tbl)["counters"] for place, tbl in KERNELS] + [run(g, case, "GRID_LDS", False, general=True)["counters"]]
        assert all(s == seen[0] for s in seen), (case, seen)
        out[case] = {k: int(v) for k, v in seen[0].items()}
        assert all(out[case][k] == seen[0][k] for k in out[case]), (case, seen[0])   # (whole numbers)
        print(case, out[case], flush=True)
        g.finalize_Integrator()
    path = os.environ.get("UNIFORM_EVENT_WORK_OUT", GOLDEN)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
