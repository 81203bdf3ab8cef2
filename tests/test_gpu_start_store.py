"""The specialised flux kernels start their photons a wavefront at a time (photon_kernel, STORE; StartSlot, csrc/tracer.hpp): a wave works
out block 0 of up to 64 consecutive photon numbers at once and a lane that turns over reads its photon's slot.

A photon's path depends on its number and the key alone, so the kernel under test must give what the general flux kernel -- which
starts every photon in its event phase, as all kernels did -- gives on the same launch: every work counter equal, fluxUp and fluxDown
equal element for element.  The domains are conservative (omega = 1) over a black or a white surface: every tallied weight is 1.0, the
float64 sums are whole numbers whatever their order, and every comparison here is `==`.

Two small domains with irregular z edges: a step cloud of 4 x 1 x 3 cells, and 5 x 3 x 2 cells so that the y index is live.  Each
launch runs once on the kernel under test and once on the general kernel (set_tuning(kernel="general"), the knob of
tests/kernel_matrix.py); kernel_name() says which ran."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests.philox_ref import philox4x32_10

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = (31, 7)
SUN = (0.8, 40.0)


def _domain(which):
    if which == "4x1x3":
        nx, ny, ze, albedo = 4, 1, [0.0, 0.3, 0.55, 1.0], 0.0
        ext = np.zeros((3, 1, 4), f32)
        ext[1:, 0, :2], ext[1:, 0, 2:] = f32(2.0), f32(18.0)          # the step cloud's two halves, clear air below
    else:
        nx, ny, ze, albedo = 5, 3, [0.0, 0.7, 1.0], 1.0
        ext = np.zeros((2, 3, 5), f32)
        ext[1] = (f32(1.0) + np.arange(15, dtype=f32).reshape(3, 5)) * f32(0.8)   # every column its own cloud: one run each (column records)
    d = dict(xe=(f32(0.5) * np.arange(nx + 1)).astype(f32), ye=(f32(0.5) * np.arange(ny + 1)).astype(f32), ze=np.array(ze, f32), ext=ext,
             ssa=np.ones(ext.shape, f32), pf=np.ones(ext.shape, np.int32))
    return d, albedo


def _integrator(which):
    from tests.test_gpu_parity import make_gpu

    d, albedo = _domain(which)
    g = make_gpu(d, M.PhaseFunctionTable([M.henyey_greenstein(0.85, 32)]), surfaceAlbedo=albedo)
    return g, d


def _name(place, tbl=False, general=False):
    return f"photon_kernel<PhiloxStream, false, {'true' if general else 'false'}, {place}{', table in LDS' if tbl else ''}>"


KNOB = {"GRID_LDS": "auto", "GRID_GLOBAL": "linear", "GRID_COLUMNS": "columns"}


def _launch(g, n, first):
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*SUN, n), firstPhoton=first)
    return g.finish()


def _pair(g, place, tbl, n, first=0, blocks=0):
    """one launch on the kernel under test and on the general kernel: both runs, the first one's plan"""
    g.select_grid_place(KNOB[place])
    g.set_tuning(blocksPerCU=blocks, kernel="auto" if tbl else "lane")
    got = _launch(g, n, first)
    assert g.kernel_name() == _name(place, tbl), g.kernel_name()
    plan = g.last_plan()
    assert plan["startStoreBytes"] == (16 if tbl else 4) * 1024 and plan["tableInLds"] == (1 if tbl else 0), plan
    g.set_tuning(blocksPerCU=blocks, kernel="general")
    ref = _launch(g, n, first)
    assert g.kernel_name() == _name(place, general=True), g.kernel_name()
    assert g.last_plan()["startStoreBytes"] == 0, g.last_plan()
    return got, ref, plan


def _equal(g, got, ref, n, what):
    assert got["counters"] == ref["counters"], (what, got["counters"], ref["counters"])
    assert got["counters"]["photons"] == n, (what, got["counters"])
    lay, ncol = g.layout(), g.nx * g.ny
    for key, at in (("fluxUp", lay.fluxUp), ("fluxDown", lay.fluxDown)):
        a, b = got["raw"][at:at + ncol], ref["raw"][at:at + ncol]
        assert (a == b).all(), (what, key, a, b)
        assert (a == np.round(a)).all(), (what, key, a)                      # whole weights: the sums are exact
    assert (got["raw"] == ref["raw"]).all(), what
    c = got["counters"]
    if "4x1x3" in str(what):    # (black surface: a photon ends at the top or at the surface, unless the tracer drops it -- a few in a million)
        assert got["raw"][lay.fluxUp:lay.fluxUp + ncol].sum() + got["raw"][lay.fluxDown:lay.fluxDown + ncol].sum() == n - c["dropped"], what
    return c


# the table-in-LDS instantiation (1024 threads) and the plain one (256), the field in LDS, read linearly and as column records
GROUPS = [("4x1x3", "GRID_LDS", True), ("4x1x3", "GRID_GLOBAL", False), ("5x3x2", "GRID_LDS", False), ("5x3x2", "GRID_COLUMNS", True),
          ("5x3x2", "GRID_GLOBAL", True), ("4x1x3", "GRID_COLUMNS", False)]
IDS = [f"{w} {p}{' table in LDS' if t else ''}" for w, p, t in GROUPS]


@pytest.mark.parametrize("which,place,tbl", GROUPS, ids=IDS)
def test_photon_counts(which, place, tbl):
    """Launches of 1, 63, 64, 65 and 127 photons, of chunk - 1, chunk and chunk + 1 (the chunk a wave takes per visit of the work counter,
    read from the plan: the last leaves a wave a fill of ONE slot), and of 4 chunks + 1: first and last fills, short fills, waves that get
    nothing.  Every photon is counted and none twice."""
    g, _ = _integrator(which)
    _, _, plan = _pair(g, place, tbl, 1)
    chunk = plan["chunk"]
    assert chunk >= 64, plan
    scat = 0
    for n in sorted({1, 63, 64, 65, 127, chunk - 1, chunk, chunk + 1, 4 * chunk + 1}):
        got, ref, plan = _pair(g, place, tbl, n)
        assert plan["chunk"] == chunk, (n, plan)
        scat += _equal(g, got, ref, n, (which, place, tbl, n))["scatterings"]
    assert scat > 0
    g.finalize_Integrator()


@pytest.mark.parametrize("which,place,tbl", GROUPS[:2], ids=IDS[:2])
def test_a_chunk_that_is_no_multiple_of_the_store(which, place, tbl):
    """One workgroup per compute unit and enough photons that a wave's chunk lies between one and four stores and is a multiple of
    none: a reservoir is drained by fills of 64 slots and a shorter one, many times per wave, the refills in between.  The photon
    count is found from the chunks the plan reports (launches of the kernel under test alone), whatever the device's size and the
    host's rule for the chunk: a chunk between its bounds is proportional to the photon count."""
    g, _ = _integrator(which)
    g.select_grid_place(KNOB[place])
    g.set_tuning(blocksPerCU=1, kernel="auto" if tbl else "lane")
    n, chunk = 400_000, 0
    for _ in range(12):
        _launch(g, n, 0)
        chunk = g.last_plan()["chunk"]
        if 64 < chunk < 256 and chunk % 64 != 0:
            break
        # (at a bound the chunk says only "too few" / "too many"; in between, aim for a chunk of 100)
        n = 2 * n if chunk <= 64 else (n // 3 if chunk >= 256 else n * 100 // chunk)
    assert 64 < chunk < 256 and chunk % 64 != 0, (n, chunk)
    n += 17
    got, ref, plan = _pair(g, place, tbl, n, blocks=1)
    assert 64 < plan["chunk"] < 256 and plan["chunk"] % 64 != 0, plan
    assert _equal(g, got, ref, n, (which, place, tbl, n))["scatterings"] > n
    g.finalize_Integrator()


@pytest.mark.parametrize("which,place,tbl", GROUPS[:3], ids=IDS[:3])
def test_photon_numbers_across_two_to_the_32(which, place, tbl):
    """firstPhoton = 2^32 - 100 and 300 photons: the fill's photon numbers carry into the counter's second word inside one store."""
    g, _ = _integrator(which)
    first, n = 2 ** 32 - 100, 300
    got, ref, _ = _pair(g, place, tbl, n, first=first)
    _equal(g, got, ref, n, (which, place, tbl, "carry"))
    low, _, _ = _pair(g, place, tbl, n, first=0)
    assert (low["raw"] != got["raw"]).any()          # (the high word is part of the photon's stream: other photons, another result)
    g.finalize_Integrator()


# Photon numbers below 2^32 whose first deviate (the start's x) or second (y) is 1.0, key SEED: found with a scan of the Philox blocks on
# the CPU (photon numbers up to 6.3e7; the 129 largest words of 2^32 give the float 1.0); test_edge_starts holds every one of them
# against tests/philox_ref.py before it is launched.  (photon number, the word: 0 the start's x, 1 its y.)  On these domains -- edges at
# whole multiples of the cell size 0.5 -- the far edge is the only one a start can lie within spacing() of: below an inner edge the
# nearest float is a whole spacing() away, and a start ON one belongs to the next cell, whose own far edge is half a unit off.
EDGE_PHOTONS = [(13015672, 0), (51380125, 0), (35430566, 1)]


def _unit(u):
    return f32(np.float64(u) / 4294967295.0)


@pytest.mark.parametrize("which,place,tbl", GROUPS[:3], ids=IDS[:3])
def test_edge_starts(which, place, tbl):
    """A photon that starts ON the far x (or y) edge -- its deviate is 1.0, so its position is xMax itself, within spacing() of the last
    edge -- takes the `i + 1` path and wraps to column 1: launched alone through firstPhoton, and with the 70 photon numbers around it."""
    assert EDGE_PHOTONS
    g, d = _integrator(which)
    seen_x = 0
    for p, word in EDGE_PHOTONS:
        block = philox4x32_10((p & 0xFFFFFFFF, p >> 32, 0, 0), SEED)
        assert _unit(block[word]) == f32(1.0), (p, block)
        x = f32(d["xe"][0] + _unit(block[0]) * f32(d["xe"][-1] - d["xe"][0]))
        seen_x += int(x == d["xe"][-1])
        for first, n in ((p, 1), (p - 30, 70)):
            got, ref, _ = _pair(g, place, tbl, n, first=first)
            _equal(g, got, ref, n, (which, place, tbl, "edge", p, n))
    assert seen_x > 0
    g.finalize_Integrator()


def test_kernels_outside_the_scope_have_no_store():
    """The bricked flux kernel (its photons come from the slab-sorted list) and a fused launch on the same domain report no store bytes,
    and the dynamic LDS they always had; both still equal the general kernel."""
    g, _ = _integrator("5x3x2")
    n = 3001
    g.select_grid_place("bricks")
    g.set_tuning(kernel="lane")
    got = _launch(g, n, 0)
    assert g.kernel_name() == _name("GRID_BRICKS"), g.kernel_name()
    plan = g.last_plan()
    assert plan["startStoreBytes"] == 0 and plan["ldsBytes"] < 1024, plan
    g.set_tuning(kernel="general")
    ref = _launch(g, n, 0)
    assert g.kernel_name() == _name("GRID_BRICKS", general=True), g.kernel_name()
    _equal(g, got, ref, n, "bricks")
    # fused: two batches in one grid, each against its own plain launch on the general kernel
    g.select_grid_place("linear")
    g.set_tuning(kernel="lane")
    g.set_batch_fusion(1)
    rs = g.computeRadiativeTransferBatches(SEED, 2, *SUN, n)
    plan = g.last_plan()
    assert "PhiloxBatchStream" in g.kernel_name() and plan["fusedBatches"] == 2 and plan["startStoreBytes"] == 0, (g.kernel_name(), plan)
    # ... and its dynamic LDS is the carve-up without a store, to the byte (the host's own lds_plan; the fused kernel keeps the table in LDS)
    from i3rc_monte_carlo_model_amd import binding as B

    table = g._inv_size[0] if plan["tableInLds"] else 0
    q = np.array([g.nx, g.ny, g.nz, 1, 0, plan["ldsTallies"], 0, 0, 0, 0, 0, 0, plan["place"], 0, 16 if table else 4, table, plan["ldsVolume"], 0], np.int32)
    out = np.zeros(13, np.int32)
    assert B.load().i3rc_hip_lds_plan_words(q.ctypes.data_as(B.ip), len(q), out.ctypes.data_as(B.ip), len(out)) == 0
    assert plan["place"] == 1 and plan["ldsBytes"] == (4 * int(out[10]) + 15) // 16 * 16, (plan, out.tolist(), table)
    g.set_batch_fusion(0)
    g.set_tuning(kernel="general")
    for k, r in enumerate(rs):
        g.launch(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*SUN, n), firstPhoton=0)
        ref = g.finish()
        assert r["counters"] == ref["counters"], (k, r["counters"], ref["counters"])
        lay = g.layout()
        assert (r["raw"][lay.fluxUp:lay.fluxAbsorbed] == ref["raw"][lay.fluxUp:lay.fluxAbsorbed]).all(), k
    g.finalize_Integrator()
