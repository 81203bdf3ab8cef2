"""How the photon step of the specialised flux kernels of plain launches (photon_kernel, STORE; csrc/kernels.hpp, csrc/tracer.hpp) spells
its addresses and its outcome: the extinction read through the biased-base address of csrc/cell_address.hpp (the indices' three `- 1` and
the base in one launch-uniform constant -- the LDS address, the global pointer, the column records' buffer descriptor), the lane state
after the step as one chain of selects on the step's own masks (arrived, above the top, below the bottom), the error exit behind one
uniform branch.  None of that may show: on every case each of the six kernels -- the field in LDS, read linearly and as column records,
each without and with the inverse table in LDS -- gives what the general flux kernel gives on the same launch: all eleven counters and
every element of the raw tally buffer with `==`.

A wrong bias or offset shows first in the last row, column and layer; every cell has its own extinction (in the largest field: another one
than each of its neighbours), so a read of the wrong cell changes where photons scatter, hence the counters.  The domains:
  1 x 1 x 1, 1 x 1 x 5          no other cell to read: the bias alone (its constant exceeds the field)
  3 x 5 x 7                     odd sizes, nx ny = 15
  32 x 1 x 16                   the step cloud's shape
  7 x 5 x k                     the largest field plan_launch still places in LDS: k from the recorded launches of tests/golden/launch_plans.json
                                (rows edge/ldsGrid/k: the last k whose plan has the field in LDS)
  3 x 5 x 7 and 33 x 31 x 3     the field in global memory, linear and as column records (33 x 31: no power of two, more columns than a wavefront)
The field in LDS runs on the first five; the other two places on the last two.  Column records hold ONE run of one value per column, so a
field that differs in every cell has none: for that place the two domains come in their column form -- every column its own value over
its own run of layers, nothing outside it --, in which a read of the wrong column gives another value or another run.

The state mapping: a surface albedo of 0 -- a photon that steps out through the bottom ends, like one that leaves through the top -- and
of 0.5 -- it is reflected and goes on --, under a sun at mu0 = 0.5, azimuth 40 degrees, so that the top and both pairs of side walls are
crossed; 20 000 photons per launch.  No absorption in the cells (omega = 1), so a photon's weight is 0.5^k and the float64 sums are exact
in any order (a weight below 2^-40 would take 40 reflections through an optical depth above 1): `==` is the right comparison.  `dropped`
(the error exit) is compared like the other counters; nothing here tries to provoke it."""
import json
import os

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from i3rc_monte_carlo_model_amd import binding as B
from tools import record_event_bookkeeping as R

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (37, 11)
SUN = (0.5, 40.0)
PHOTONS = 20000
ALBEDOS = (0.0, 0.5)


def largest_lds_layers():
    """the last k of the recorded rows edge/ldsGrid/k (7 x 5 x k) whose launch had the field in LDS"""
    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
        golden = json.load(f)
    on = golden["plan_names"].index("ldsGrid")
    ks = [int(rid.split("/")[2]) for rid, row in golden["rows"].items()
          if rid.startswith("edge/ldsGrid/") and rid.count("/") == 2 and "plan" in row and row["plan"][on] == 1]
    assert ks, "no recorded launch with the field in LDS"
    return max(ks)


SHAPES = {"1x1x1": (1, 1, 1), "1x1x5": (1, 1, 5), "3x5x7": (3, 5, 7), "32x1x16": (32, 1, 16), "largest": (7, 5, largest_lds_layers()),
          "33x31x3": (33, 31, 3), "3x5x7 columns": (3, 5, 7), "33x31x3 columns": (33, 31, 3)}
# place of the field -> the domains its two kernels run on
DOMAINS = {"GRID_LDS": ("1x1x1", "1x1x5", "3x5x7", "32x1x16", "largest"), "GRID_GLOBAL": ("3x5x7", "33x31x3"),
           "GRID_COLUMNS": ("3x5x7 columns", "33x31x3 columns")}
IDS = [f"{p}{' table in LDS' if t else ''}" for p, t in R.KERNELS]


def domain(which):
    """regular x / y edges 0.25 apart, layers of two alternating depths that add up to 1 in all; extinction 0.6 ... 2.4, each cell its
    own (the largest field: per column and by layer parity -- every cell differs from its neighbours): optical depth 0.6 ... 2.4"""
    nx, ny, nz = SHAPES[which]
    dz = np.where(np.arange(nz) % 2 == 0, 1.5, 0.5)
    ze = np.concatenate([[0.0], np.cumsum(dz / dz.sum())]).astype(f32)
    n = nx * ny * nz
    if which.endswith("columns"):   # column c: three times 0.6 + 1.8 c / (columns - 1) from layer c % nz on, over 1 ... nz - c % nz layers
        c = np.arange(nx * ny).reshape(1, ny, nx)
        lo = c % nz
        hi = lo + (c // nz) % (nz - lo)
        z = np.arange(nz).reshape(nz, 1, 1)
        ext = np.where((z >= lo) & (z <= hi), f32(0.6) + f32(1.8) * c.astype(f32) / f32(nx * ny - 1), f32(0.0)) * f32(3.0)
    elif which == "largest":
        ext = (f32(0.6) + f32(1.8 / 70.0) * (np.arange(nx * ny, dtype=f32).reshape(1, ny, nx) + f32(35.0) * (np.arange(nz, dtype=f32) % 2).reshape(nz, 1, 1)))
    else:
        ext = (f32(0.6) + f32(1.8) * np.arange(n, dtype=f32) / f32(max(n - 1, 1))).reshape(nz, ny, nx)
    ext = ext.astype(f32)
    return dict(xe=(f32(0.25) * np.arange(nx + 1)).astype(f32), ye=(f32(0.25) * np.arange(ny + 1)).astype(f32), ze=ze, ext=ext,
                ssa=np.ones(ext.shape, f32), pf=np.ones(ext.shape, np.int32))


def integrator(which, albedo):
    d = domain(which)
    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    dom.addOpticalComponent("cloud", d["ext"], d["ssa"], d["pf"], M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]))
    g = M.new_Integrator(dom)
    g.specifyParameters(surfaceAlbedo=albedo, useRussianRoulette=False)
    return g


def run(g, place, tbl, general=False):
    """one launch on one of the six kernels, or on the general kernel at the same place of the field; the kernel's name is returned"""
    g.select_grid_place(R.KNOB[place])
    g.set_tuning(kernel="general" if general else ("auto" if tbl else "lane"))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*SUN, PHOTONS), firstPhoton=0)
    res = g.finish()
    return res, g.kernel_name()


@pytest.fixture(scope="module")
def general():
    """the general kernel's result of every case at every place of the field: computed once, shared, never written to"""
    out = {}
    for place, names in DOMAINS.items():
        for which in names:
            for albedo in ALBEDOS:
                g = integrator(which, albedo)
                res, name = run(g, place, False, general=True)
                g.finalize_Integrator()
                assert name == R.kernel_name(place, False, True), name
                res["raw"].setflags(write=False)
                out[which, albedo, place] = res
    return out


def test_the_cases_reach_every_boundary(general):
    """what the cases are for: photons leave through the top and arrive at the surface, a reflecting surface sends them on (more traces
    than scatterings and photons), and where a domain has more than one cell a trace makes more than one voxel step on average"""
    for (which, albedo, place), res in general.items():
        n = res["counters"]
        assert n["photons"] == PHOTONS and n["exitsTop"] > 0 and n["surfaceHits"] > 0 and n["scatterings"] > 0, (which, albedo, place, n)
        if albedo > 0.0:
            assert n["tracerCalls"] > n["scatterings"] + n["photons"], (which, albedo, place, n)
        else:
            assert n["tracerCalls"] == n["scatterings"] + n["photons"], (which, albedo, place, n)
        if which != "1x1x1":
            assert n["cellSteps"] > n["tracerCalls"], (which, albedo, place, n)
    # the two albedos part at the bottom: the same photons, other fates
    for place, names in DOMAINS.items():
        for which in names:
            assert general[which, 0.0, place]["counters"]["surfaceHits"] < general[which, 0.5, place]["counters"]["surfaceHits"]


@pytest.mark.parametrize("place,tbl", R.KERNELS, ids=IDS)
def test_kernel_equals_general_kernel(place, tbl, general):
    for which in DOMAINS[place]:
        for albedo in ALBEDOS:
            g = integrator(which, albedo)
            got, name = run(g, place, tbl)
            g.finalize_Integrator()
            ref = general[which, albedo, place]
            what = (which, albedo, place, tbl)
            # (the largest field in LDS leaves no room for the inverse table beside it: there the launch with the table asked for runs the
            # kernel without -- the same kernel a second time, which the name says)
            want = R.kernel_name(place, tbl and which != "largest")
            assert name == want, (what, name)
            assert sorted(got["counters"]) == sorted(B.COUNTER_NAMES), what
            print(what, got["counters"])
            for k in B.COUNTER_NAMES:
                assert got["counters"][k] == ref["counters"][k], (what, k, got["counters"], ref["counters"])
            assert got["raw"].shape == ref["raw"].shape and (got["raw"] == ref["raw"]).all(), (what, np.flatnonzero(got["raw"] != ref["raw"]))
            n = got["counters"]
            assert n["tracerCalls"] == n["scatterings"] + n["surfaceHits"] + n["exitsTop"] + n["dropped"], (what, n)
