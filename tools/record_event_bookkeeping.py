"""The cases of tests/test_gpu_event_bookkeeping.py, and the recorder of their work counters.

The specialised flux kernels of plain launches (photon_kernel, STORE) derive some of their work counters from others and take the rest
from the masks of the event phase; the general kernel shares that code's neighbourhood, so the counters are also pinned to what the
commit BEFORE that change counted: run there, once, on a GPU,
  python3 tools/record_event_bookkeeping.py            -> tests/golden/event_bookkeeping_parent.json
writes the eleven counters (binding.COUNTER_NAMES) of every case, after checking that all six kernels and the general kernel agree on
them.  The test imports CASES, integrator() and run() from here, so that the recorded launches and the tested ones are the same."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import i3rc_monte_carlo_model_amd as M   # noqa: E402

f32 = np.float32
SEED = (29, 5)
GOLDEN = os.path.join(ROOT, "tests", "golden", "event_bookkeeping_parent.json")
# the six kernels in scope: the field in LDS, read linearly and as column records, each without and with the inverse table in LDS
KERNELS = [(place, tbl) for place in ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS") for tbl in (False, True)]
KNOB = {"GRID_LDS": "auto", "GRID_GLOBAL": "linear", "GRID_COLUMNS": "columns"}

# name: domain, photons, single-scattering albedo, surface albedo, Russian roulette, (mu0, phi)
CASES = {
    "a": dict(domain="3x2x4", photons=4097, ssa=1.0, albedo=0.0, roulette=False, sun=(1.0, 0.0)),
    "b": dict(domain="step16", photons=20001, ssa=1.0, albedo=0.0, roulette=False, sun=(1.0, 0.0)),
    "c": dict(domain="3x2x4", photons=4097, ssa=1.0, albedo=0.3, roulette=False, sun=(1.0, 0.0)),
    "d-roulette": dict(domain="3x2x4", photons=4097, ssa=0.9, albedo=0.0, roulette=True, sun=(1.0, 0.0)),
    "d-plain": dict(domain="3x2x4", photons=4097, ssa=0.9, albedo=0.0, roulette=False, sun=(1.0, 0.0)),
    "e": dict(domain="3x2x4", photons=4097, ssa=1.0, albedo=0.0, roulette=False, sun=(0.35, 40.0)),
}


def domain(which, ssa):
    if which == "step16":
        from tools import cases

        return cases.step_cloud(ssa=ssa, nlayers=16), 64
    # 3 x 2 x 4 cells, irregular layers, clear air below; every column its own cloud of optical depth 0.7 ... 2.2: a photon scatters a
    # few times, so that the weights of cases c and d stay above 2^-16 and their float64 sums are exact whatever the order
    nx, ny = 3, 2
    ext = np.zeros((4, ny, nx), f32)
    ext[1:] = (f32(1.0) + f32(0.4) * np.arange(nx * ny, dtype=f32).reshape(ny, nx))[None]
    d = dict(xe=(f32(0.5) * np.arange(nx + 1)).astype(f32), ye=(f32(0.5) * np.arange(ny + 1)).astype(f32),
             ze=np.array([0.0, 0.3, 0.45, 0.8, 1.0], f32), ext=ext, ssa=np.full(ext.shape, f32(ssa)), pf=np.ones(ext.shape, np.int32))
    return d, 32


def integrator(case):
    c = CASES[case]
    d, moments = domain(c["domain"], c["ssa"])
    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    dom.addOpticalComponent("cloud", d["ext"], d["ssa"], d["pf"], M.PhaseFunctionTable([M.henyey_greenstein(0.85, moments)]))
    g = M.new_Integrator(dom)
    g.specifyParameters(surfaceAlbedo=c["albedo"], useRussianRoulette=c["roulette"])
    return g


def kernel_name(place, tbl=False, general=False):
    return f"photon_kernel<PhiloxStream, false, {'true' if general else 'false'}, {place}{', table in LDS' if tbl else ''}>"


def run(g, case, place, tbl, general=False):
    """one launch of the case on one of the six kernels, or on the general kernel at the same place of the field"""
    c = CASES[case]
    g.select_grid_place(KNOB[place])
    g.set_tuning(kernel="general" if general else ("auto" if tbl else "lane"))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*c["sun"], c["photons"]), firstPhoton=0)
    res = g.finish()
    assert g.kernel_name() == kernel_name(place, tbl and not general, general), g.kernel_name()
    return res


# ---- launches whose weights only halve (absorption without roulette): the rules tests/test_gpu_scalar_relief.py states in its text,
# here for the tests that share them (tests/test_gpu_first_flight.py).  A launch is (surface albedo, roulette, photons, ...), a
# setting (domain, single-scattering albedo, ...).
RERUNS = 3                       # runs of the general kernel where a launch's sums may depend on the order
MAX_SPREAD = 16 * 2.0 ** -52     # what the reference's own runs may differ by, relative, in any word


def weights_only_halve(setting, launch):
    """absorption and no roulette: weights that halve without end"""
    return setting[1] == 0.5 and not launch[1]


def provably_exact(launch, counters):
    """every partial sum of every tally word of the launch fits a float64: addends 2^-j with j <= scatterings + surfaceHits + 1 of
    the whole launch, no word above 2 photons"""
    return counters["scatterings"] + counters["surfaceHits"] + 1 + np.log2(2.0 * launch[2]) <= 53


def spread_of(runs):
    """largest relative difference of a word among runs of one launch; 0.0: equal word for word"""
    worst = 0.0
    for i in range(len(runs)):
        for j in range(i):
            bad = runs[i] != runs[j]
            if bad.any():
                worst = max(worst, float((np.abs(runs[i] - runs[j])[bad] / np.maximum(np.abs(runs[i][bad]), np.abs(runs[j][bad]))).max()))
    return worst


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
    path = os.environ.get("EVENT_BOOKKEEPING_OUT", GOLDEN)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
