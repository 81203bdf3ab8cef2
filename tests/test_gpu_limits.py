"""The kernels at the limits the host code sets at run time: fields packed into fixed widths, LDS regions sized from budgets.

An off-by-one at any of them changes tallies without a fault, and a 3-sigma test cannot see it.  Each test takes the last value a
limit accepts and the first past it (refused on the host, or sent to another path), proves from i3rc_hip_last_plan or the work
counters that it reached the side it claims, and compares the runs with the plainest launch of the same photons -- the general
kernel, the field read linearly, every tally straight to global memory, one launch per batch -- or with an exact invariance: identical
work counters, tallies equal up to the order of their float64 additions (tests/sums.py)."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from i3rc_monte_carlo_model_amd.binding import I3RCError
from tests.sums import assert_same_sums

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = (23, 9)
N = 30_001                      # a multiple of neither the 256-photon chunk nor the 1024-thread workgroup
SUN = (0.7, 30.0)
PHOTON_SIDE = ("photons", "dropped", "scatterings", "surfaceHits", "exitsTop", "roulette")


def _hg(*gs, n=32):
    return M.PhaseFunctionTable([M.henyey_greenstein(g, n) for g in gs])


def _make(d, tables, **params):
    from tests.test_gpu_parity import make_gpu

    return make_gpu(d, tables, **params)


def _run(g, n=N, k=0, seed=SEED):
    return g.computeRadiativeTransfer(M.new_RandomNumberSequence((seed[0], seed[1] + k)), M.new_PhotonStream(*SUN, n))


def _plainest(g):
    g.set_batch_fusion(0)
    g.set_tuning(kernel="general")
    g.select_grid_place("linear")
    g.set_lds_tallies(False)


def _same(a, b, nd=0, what=None):
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    assert_same_sums(a["raw"], b["raw"], a["counters"], directions=nd, what=what)


def _box(nx, ny, nz, ssa=0.9, seed=1, depth=3.0, regular=False):
    """an absorbing cloud on odd-sized, irregular (or regular) x / y edges: every cell its own extinction"""
    rng = np.random.default_rng(seed)
    if regular:
        xe, ye = (f32(30.0) * np.arange(nx + 1)).astype(f32), (f32(30.0) * np.arange(ny + 1)).astype(f32)
    else:
        xe = np.concatenate([[0.0], np.cumsum(rng.uniform(20, 40, nx))]).astype(f32)
        ye = np.concatenate([[0.0], np.cumsum(rng.uniform(20, 40, ny))]).astype(f32)
    ze = np.linspace(0.0, 300.0, nz + 1).astype(f32)
    ext = (rng.uniform(0.2, 1.0, (nz, ny, nx)) * depth / 300.0).astype(f32)
    return dict(xe=xe, ye=ye, ze=ze, ext=ext, ssa=np.full(ext.shape, f32(ssa)), pf=np.ones(ext.shape, np.int32))


# ---- 1. LDS budgets ---------------------------------------------------------------------------------------------------------------
def _edge(make, flag, lo, hi):
    """Bisection on a size k of the shape make(k): the last k whose 1-photon launch has plan[flag] on and the first where it is off.
    The test asserts that both sides were found, from the plan each launch reports."""
    def on(k):
        g = make(k)
        _run(g, n=1)
        v = g.last_plan()[flag]
        g.finalize_Integrator()
        return v == 1
    assert on(lo) and not on(hi), (flag, lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if on(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


RAD2 = dict(intensityMus=[0.9, 0.5], intensityPhis=[0.0, 120.0], useRussianRouletteForIntensity=True, zetaMin=0.3)
LDS_CASES = {
    # flag: (shape of size k, parameters, bisection range)
    "ldsTallies": (lambda k: _box(2 * k + 1, 3, 2), dict(surfaceAlbedo=0.3), 1, 1200),
    "ldsVolume": (lambda k: _box(5, 3, k), dict(surfaceAlbedo=0.3), 1, 400),
    "ldsIntensity": (lambda k: _box(2 * k + 1, 3, 2), dict(RAD2, surfaceAlbedo=0.3), 1, 200),
    "ldsGrid": (lambda k: _box(7, 5, k), dict(surfaceAlbedo=0.3), 1, 2000),
    # (the table-in-LDS kernels are the common class's: regular x / y.  Conservative, so that no volume tallies come and go on the
    # way: the flag is on up to the edge, off beyond it while the field is in LDS, and on again once the field has left LDS)
    "tableInLds": (lambda k: _box(7, 5, k, ssa=1.0, regular=True), dict(surfaceAlbedo=0.3), 1, 350),
}


@pytest.mark.parametrize("flag", sorted(LDS_CASES))
def test_lds_budget_boundaries(flag):
    """Each LDS region at the last shape that has it and the first that does not (found by bisection on the plan of 1-photon
    launches): both shapes against the plainest launch of 30 001 photons.  Probed (size k of LDS_CASES): ldsTallies on at 314, off at
    315 (629 / 631 x 3 columns); ldsVolume 261 / 262 layers of 5 x 3; ldsIntensity 84 / 85 (169 / 171 x 3 columns, two directions);
    ldsGrid 450 / 451 layers of 7 x 5; the inverse table in LDS 193 / 194 layers of 7 x 5 (307 / 308 before the waves' start stores came
    to lie beside the table).  Each found pair is printed; tests/test_launch_plan_cpu.py asserts the pairs from recorded launches."""
    make, params, lo, hi = LDS_CASES[flag]
    tabs = _hg(0.85)
    last_on, first_off = _edge(lambda k: _make(make(k), tabs, **params), flag, lo, hi)
    print(f"{flag}: on at size {last_on}, off at {first_off}")
    nd = len(params.get("intensityMus", []))
    for k, want in ((last_on, 1), (first_off, 0)):
        g = _make(make(k), tabs, **params)
        got = _run(g)
        plan = g.last_plan()
        assert plan[flag] == want, (flag, k, plan)
        assert got["counters"]["scatterings"] > 0
        _plainest(g)
        ref = _run(g)
        assert g.last_plan()[flag] == 0 and "GRID_GLOBAL" in g.kernel_name(), (flag, g.last_plan(), g.kernel_name())
        _same(got, ref, nd, (flag, k, plan))
        g.finalize_Integrator()


# ---- 2. packed fields -------------------------------------------------------------------------------------------------------------
AGREE = (0, 1, 127, 128, 253, 254)


def _directions(seed):
    rng = np.random.default_rng(seed)
    mus = rng.uniform(0.2, 1.0, 255).astype(f32)
    phis = rng.uniform(0.0, 360.0, 255).astype(f32)
    for i, (m, p) in zip(AGREE, ((1.0, 0.0), (0.5, 30.0), (0.8, 200.0), (0.3, 90.0), (0.95, 310.0), (0.6, 45.0))):
        mus[i], phis[i] = m, p
    return mus, phis


def _int_block(g, raw, nd, idx):
    lay = g.layout()
    ncol = g.nx * g.ny
    b = raw[lay.intensityByComponent:lay.intensityByComponent + (g.ncomp + 1) * nd * ncol].reshape(g.ncomp + 1, nd, ncol)
    return b[:, list(idx)]


def _flux_block(g, raw):
    lay = g.layout()
    return raw[lay.fluxUp:lay.intensityByComponent]


@pytest.mark.parametrize("extra", [dict(), dict(useHybridPhaseFunsForIntenCalcs=True, hybridPhaseFunWidth=7.0, numOrdersOrigPhaseFunIntenCalcs=1,
                                                 limitIntensityContributions=True, maxIntensityContribution=0.5)], ids=["plain", "hybrid+limit"])
def test_255_directions(extra):
    """Direction index in 8 bits of a ray's info word: 255 directions (the last accepted) and 256 (refused).  Two lists that agree
    only at {0, 1, 127, 128, 253, 254} give the same photons -- a ray's deviates are keyed by (photon, event block, direction + 1),
    a photon's own by (photon, block, 0) -- so the photon-side counters are identical and the tallies at those positions agree.
    The 255-direction run also equals the general kernel's."""
    from tools import cases

    d = cases.step_cloud(ssa=0.95, nlayers=8, ncolumns=16)
    base = dict(extra, useRussianRouletteForIntensity=True, zetaMin=0.3, surfaceAlbedo=0.2)
    runs = []
    for seed in (1, 2):
        mus, phis = _directions(seed)
        g = _make(d, _hg(0.85), intensityMus=mus, intensityPhis=phis, **base)
        runs.append((g, _run(g)))
    (ga, a), (gb, b) = runs
    assert len(ga.intensityDirections) == 255 and a["counters"]["raysSkipped"] + a["counters"]["shadowSteps"] > 0
    assert ", true, " in ga.kernel_name() and a["counters"]["scatterings"] > 0
    for k in PHOTON_SIDE:
        assert a["counters"][k] == b["counters"][k], (k, a["counters"], b["counters"])
    assert_same_sums(_flux_block(ga, a["raw"]), _flux_block(gb, b["raw"]), a["counters"], what="flux")
    assert_same_sums(_int_block(ga, a["raw"], 255, AGREE), _int_block(gb, b["raw"], 255, AGREE), a["counters"], directions=255, what="agreeing directions")
    if extra:
        lay = ga.layout()
        exa = a["raw"][lay.intensityExcess:lay.counters].reshape(2, 255)[:, list(AGREE)]
        exb = b["raw"][lay.intensityExcess:lay.counters].reshape(2, 255)[:, list(AGREE)]
        assert_same_sums(exa, exb, a["counters"], directions=255, what="excess")
    # ... and the general kernel on the same photons
    _plainest(ga)
    _same(a, _run(ga), 255, "general kernel")
    # 256 directions: refused, and nothing changes
    total = ga.layout().total
    with pytest.raises(I3RCError):
        ga.specifyParameters(intensityMus=np.full(256, 0.5, f32), intensityPhis=np.zeros(256, f32))
    assert len(ga.intensityDirections) == 255 and ga.layout().total == total
    _same(a, _run(ga), 255, "after the refusal")
    ga.finalize_Integrator(); gb.finalize_Integrator()


def _comps(cloud_at, ncomp=255):
    """an absorbing cloud with two table entries as component cloud_at (1-based) of ncomp, every other component empty"""
    from tools import cases

    d = cases.step_cloud(ssa=0.9, nlayers=8, ncolumns=16)
    pf = np.ones(d["ext"].shape, np.int32)
    pf[:, :, 1::3] = 2
    zero = np.zeros_like(d["ext"])
    ext = [zero] * ncomp
    ssa = [np.ones_like(zero)] * ncomp
    pfs = [np.zeros(zero.shape, np.int32)] * ncomp
    ext[cloud_at - 1], ssa[cloud_at - 1], pfs[cloud_at - 1] = d["ext"], d["ssa"], pf
    return dict(d, ext=ext, ssa=ssa, pf=pfs)


def _with_tables(d, ncomp, params):
    tab = _hg(0.85, 0.5)
    g = _make(d, [tab] * ncomp, **params)
    inv, fwd = tab.inverse_table(2001), tab.forward_table(361)
    for c in range(ncomp):
        g.set_tables(c + 1, inverse=inv, forward=fwd if params.get("intensityMus") is not None else None)
    return g


@pytest.mark.parametrize("mode", ["ring", "one direction", "fused"])
def test_255_components(mode):
    """Component number in 8 bits: a cloud as component 1 or as component 255 of 255 (254 empty ones around it).  The selection
    deviate is drawn either way and always picks the cloud: identical counters, the same flux tallies, and intensityByComponent[1]
    of one run equal to [255] of the other.  256 components are refused at create."""
    params = dict(surfaceAlbedo=0.2, useRussianRouletteForIntensity=True, zetaMin=0.3)
    if mode == "ring":
        params.update(intensityMus=[0.9, 0.4, 0.7], intensityPhis=[0.0, 100.0, 250.0])
    elif mode == "one direction":
        params.update(intensityMus=[0.8], intensityPhis=[40.0])
    nd = len(params.get("intensityMus", []))
    out = []
    for at in (1, 255):
        g = _with_tables(_comps(at), 255, params)
        if mode == "fused":
            g.set_batch_fusion(1)
            rs = g.computeRadiativeTransferBatches(SEED, 2, *SUN, 7001)
            assert g.last_plan()["fusedBatches"] == 2, g.last_plan()
        else:
            rs = [_run(g)]
        assert g.ncomp == 255
        out.append((g, rs))
    (ga, ra), (gb, rb) = out
    if mode == "one direction":
        assert "one direction" in ga.kernel_name(), ga.kernel_name()
    elif mode == "ring":
        assert ", true, false, " in ga.kernel_name() and "wide" in ga.kernel_name() and "one direction" not in ga.kernel_name(), ga.kernel_name()
    for a, b in zip(ra, rb):
        assert a["counters"] == b["counters"], (a["counters"], b["counters"])
        assert a["counters"]["scatterings"] > 0 and a["volumeAbsorption"].sum() > 0
        assert_same_sums(_flux_block(ga, a["raw"]), _flux_block(gb, b["raw"]), a["counters"], what="flux")
        if nd:
            ia, ib = _int_block(ga, a["raw"], nd, range(nd)), _int_block(gb, b["raw"], nd, range(nd))
            assert ia[1].any()
            assert_same_sums(ia[[0, 1]], ib[[0, 255]], a["counters"], directions=nd, what="by component")
            assert not ia[2:].any() and not ib[1:255].any()
    ga.finalize_Integrator(); gb.finalize_Integrator()
    with pytest.raises(I3RCError, match="ncomp"):
        _make(_comps(1, 256), [_hg(0.85, 0.5)] * 256)


def test_radiance_table_entry_65535():
    """Table entry in the upper 16 bits of a ray's info word: every cell on entry 65535 of a table of 65535 identical entries
    equals the 1-entry run (the repeated-table trick of test_phase_function_entries_beyond_32767); entry 65536 is refused."""
    from tools import cases

    d = cases.step_cloud(ssa=0.97, nlayers=8)
    t = _hg(0.85)
    inv, fwd = t.inverse_table(129), t.forward_table(181)
    params = dict(intensityMus=[1.0, 0.5], intensityPhis=[0.0, 30.0], useRussianRouletteForIntensity=True, zetaMin=0.3, surfaceAlbedo=0.2)
    hg = M.henyey_greenstein(0.85, 32)
    res = []
    for entries in (1, 65535, 65536):
        dd = dict(d, pf=np.full(d["ext"].shape, entries, np.int32))
        g = _make(dd, M.PhaseFunctionTable([hg] * entries), **params)
        g.set_tables(1, inverse=np.repeat(inv, entries, axis=0), forward=np.repeat(fwd, entries, axis=0))
        if entries == 65536:
            with pytest.raises(I3RCError, match="at most 65535 phase-function table entries"):
                _run(g)
        else:
            res.append(_run(g))
        g.finalize_Integrator()
    assert res[0]["counters"]["scatterings"] > 0
    _same(res[0], res[1], 2, "entry 65535")


@pytest.mark.parametrize("ncomp", [2, 3])
def test_cell_record_table_entries(ncomp):
    """Two table entries share one word of a 2- or 3-component cell record: entry 65535 in the first or the second component is
    kept as a record, 65536 is not (the plan says which), and both equal the domain on entry 1."""
    from tools import cases

    d = cases.step_cloud(ssa=0.9, nlayers=8, ncolumns=16)
    t = _hg(0.85)
    inv = t.inverse_table(129)
    hg = M.henyey_greenstein(0.85, 32)
    exts = [d["ext"], f32(0.5) * d["ext"] + f32(1e-3), np.full_like(d["ext"], f32(2e-3))][:ncomp]
    ssas = [d["ssa"], np.full_like(d["ssa"], f32(0.8)), np.ones_like(d["ssa"])][:ncomp]

    def run(comp, entry):
        pfs = [np.ones(d["ext"].shape, np.int32) for _ in range(ncomp)]
        pfs[comp] = np.full(d["ext"].shape, entry, np.int32)
        tabs = [M.PhaseFunctionTable([hg] * (entry if c == comp else 1)) for c in range(ncomp)]
        g = _make(dict(d, ext=exts, ssa=ssas, pf=pfs), tabs, surfaceAlbedo=0.3)
        for c in range(ncomp):
            g.set_tables(c + 1, inverse=np.repeat(inv, entry if c == comp else 1, axis=0))
        r = _run(g)
        plan = g.last_plan()
        g.finalize_Integrator()
        return r, plan

    ref, plan = run(0, 1)
    assert plan["cellRecordBytes"] == 16 * (ncomp - 1), plan
    assert ref["counters"]["scatterings"] > 0 and ref["volumeAbsorption"].sum() > 0
    for comp in (0, 1):
        for entry, rec in ((65535, 16 * (ncomp - 1)), (65536, 0)):
            r, plan = run(comp, entry)
            assert plan["cellRecordBytes"] == rec, (comp, entry, plan)
            _same(ref, r, 0, (comp, entry))


# ---- 3. lane counters of fused launches --------------------------------------------------------------------------------------------
def _slab(depth, ssa):
    ze = np.array([0.0, 1000.0], f32)
    ext = np.full((1, 1, 1), f32(depth / 1000.0))
    return dict(xe=np.array([0.0, 1000.0], f32), ye=np.array([0.0, 1000.0], f32), ze=ze, ext=ext,
                ssa=np.full(ext.shape, f32(ssa)), pf=np.ones(ext.shape, np.int32))


@pytest.mark.parametrize("ssa", [1.0, 0.99995], ids=["conservative", "roulette"])
def test_lane_counter_hand_over(ssa):
    """Fused flux launches count per lane, scatterings | roulette plays and surface arrivals | exits through the top as 16-bit
    pairs, handed over when a half reaches 0x8000.  One-photon batches on an optically thick slab (tau 2000): a batch with 65 536
    or more scatterings -- one photon in one lane -- can only be counted right through the hand-over; every batch's counters must
    equal those of its own plain launch.  The other halves cannot be reached by one photon: a roulette play survives with
    probability below 1/2, so 32 768 plays in one photon have probability below 2^-32768; a photon ends at its first exit through
    the top; and arrivals at a black surface end it too (a white one under a slab thick enough to keep the photon would need
    on the order of 1e9 scatterings for 32 768 arrivals).  Probed: 65 536 scatterings (two hand-overs) and the largest count the
    loop reaches (conservative: 17 of 1000 batches, the largest 660 306 scatterings; omega = 0.99995: one, 97 027)."""
    g = _make(_slab(2000.0, ssa), _hg(0.85), surfaceAlbedo=0.0)
    nb = 1000
    g.set_batch_fusion(1)
    fused = g.computeRadiativeTransferBatches(SEED, nb, *SUN, 1)
    assert g.last_plan()["fusedBatches"] == nb and "PhiloxBatchStream" in g.kernel_name(), (g.last_plan(), g.kernel_name())
    scat = [r["counters"]["scatterings"] for r in fused]
    assert max(scat) >= 65536, max(scat)
    print(f"lane counters: {sum(x >= 65536 for x in scat)} batches of 65 536 scatterings or more, the largest {max(scat):.0f}")
    if ssa < 1:
        assert sum(r["counters"]["roulette"] for r in fused) > 0
    g.set_batch_fusion(0)
    for k, r in enumerate(fused):
        p = _run(g, n=1, k=k)
        assert p["counters"] == r["counters"], (k, p["counters"], r["counters"])
    g.finalize_Integrator()


# ---- 4. more than 65535 batches in one fused group ----------------------------------------------------------------------------------
def test_more_than_65535_batches_in_one_group():
    """absorbed_columns cuts a group's tally blocks into grids of 65535: a fused loop of 70 000 one-photon batches on a 1 x 1 x 2
    absorbing column is one group (the plan says so); every batch's fluxAbsorbed is the sum of its volume column; batches 0, 1,
    65534 ... 65537 and the last equal their plain launches; the device's batch moments equal the sums of the batches' results."""
    import ctypes as C

    from i3rc_monte_carlo_model_amd import binding as B

    d = dict(xe=np.array([0.0, 100.0], f32), ye=np.array([0.0, 100.0], f32), ze=np.array([0.0, 70.0, 100.0], f32),
             ext=np.full((2, 1, 1), f32(0.02)), ssa=np.full((2, 1, 1), f32(0.6)), pf=np.ones((2, 1, 1), np.int32))
    g = _make(d, _hg(0.85), surfaceAlbedo=0.4)
    g.set_batch_fusion(1)
    nb = 70_000
    # (computeRadiativeTransferBatches' own call, without its per-batch finish(): the raw blocks of all 70 000 batches are what the
    # column sums below are taken of, and what finish() is applied to batch by batch for the moments further down)
    g._ensure_tables()
    lay = g.layout()
    raw = np.zeros((nb, lay.total), np.float64)
    s = B.Source()
    s.kind, s.solarMu, s.solarAzimuth = 0, SUN[0], SUN[1]
    g._check(g._lib.i3rc_hip_run_batches(g._h, SEED[0], SEED[1], nb, 1, C.byref(s), 0, raw.ctypes.data_as(B.dp)), "run_batches")
    assert g.last_plan()["fusedBatches"] == nb, g.last_plan()
    cnt = raw[:, lay.counters:lay.counters + B.NUM_COUNTERS]
    assert (cnt[:, B.COUNTER_NAMES.index("photons")] == 1).all()
    vol = raw[:, lay.volumeAbsorption:lay.volumeAbsorption + 2]
    assert np.array_equal(raw[:, lay.fluxAbsorbed], vol[:, 0] + vol[:, 1])
    assert (raw[65535:, lay.fluxAbsorbed] > 0).any() and (raw[:65535, lay.fluxAbsorbed] > 0).any()
    g.set_batch_fusion(0)
    for k in (0, 1, 65534, 65535, 65536, 65537, nb - 1):
        p = _run(g, n=1, k=k)
        f = g.finish(raw[k].copy())
        _same(f, p, 0, k)
    g.set_batch_fusion(1)
    s1, s2, mc = g.computeRadiativeTransferBatchMoments(SEED, nb, *SUN, 1)
    assert g.last_plan()["fusedBatches"] == nb, g.last_plan()
    assert mc["photons"] == nb and mc["scatterings"] == cnt[:, B.COUNTER_NAMES.index("scatterings")].sum()
    per = []
    for k in range(nb):
        g._results = g.finish(raw[k])   # (as test_batch_moments_on_the_device_equal_the_drivers_sums: reportResults of batch k)
        per.append(g.reportResults())
    for key in s1:
        x = np.stack([np.asarray(p[key], np.float64) for p in per])
        tol = 2e-6 if key.startswith("mean") or key == "absorbedProfile" else 1e-9
        assert np.allclose(s1[key], x.sum(0), rtol=tol, atol=1e-12), (key, np.abs(s1[key] - x.sum(0)).max())
        assert np.allclose(s2[key], (x * x).sum(0), rtol=2 * tol, atol=1e-12), key
    g.finalize_Integrator()


# ---- 5. edge vectors at the LDS hard limit -----------------------------------------------------------------------------------------
def _column(nz, ncomp=1, ssa=0.0, seed=4):
    rng = np.random.default_rng(seed)
    ze = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, nz))]).astype(f32)
    ext = (rng.uniform(0.5, 1.5, (nz, 1, 1)) * (1.5 / float(ze[-1]))).astype(f32)
    d = dict(xe=np.array([0.0, 100.0], f32), ye=np.array([0.0, 100.0], f32), ze=ze, ext=ext, ssa=np.full(ext.shape, f32(ssa)),
             pf=np.ones(ext.shape, np.int32))
    if ncomp == 2:
        d = dict(d, ext=[ext, f32(0.5) * ext], ssa=[d["ssa"], np.ones_like(d["ssa"])], pf=[d["pf"], d["pf"]])
    return d


def test_edge_vectors_at_the_lds_hard_limit():
    """The edge vectors of a 1 x 1 column with an irregular z grid at the largest nz a launch accepts (found by bisection on
    1-photon launches) and one layer more (refused by plan_launch's host check with an I3RCError).  At the edge an omega = 0 flux
    run reproduces Beer-Lambert transmission exp(-tau / mu0), tau in float64, within 4 binomial standard errors.  Probed: 40 443
    layers accepted, 40 444 refused.  (The refusal is plan_launch's, at the launch: i3rc_hip_create takes such a domain.)"""
    tab = _hg(0.85)

    def accepted(nz):
        g = _make(_column(nz), tab, surfaceAlbedo=0.0)
        try:
            _run(g, n=1)
            return True
        except I3RCError as e:
            assert "edge vectors do not fit in LDS" in str(e), e
            return False
        finally:
            g.finalize_Integrator()

    lo, hi = 30_000, 45_000
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    print(f"edge vectors: nz {lo} accepted, {hi} refused")
    d = _column(lo)
    g = _make(d, tab, surfaceAlbedo=0.0)
    n = 50_000
    r = _run(g, n=n)
    plan = g.last_plan()
    assert plan["ldsGrid"] == 0 and plan["ldsBytes"] > 150 * 1024, plan
    tau = float(np.sum(d["ext"][:, 0, 0].astype(np.float64) * np.diff(d["ze"].astype(np.float64))))
    t = np.exp(-tau / SUN[0])
    sigma = np.sqrt(t * (1 - t) / n)
    assert abs(float(r["fluxDown"].mean()) - t) <= 4 * sigma, (lo, float(r["fluxDown"].mean()), t, sigma)
    assert float(r["fluxUp"].sum()) == 0.0
    g.finalize_Integrator()
    assert hi == lo + 1


def test_trace_rays_at_its_lds_limit(oracle):
    """i3rc_hip_trace_rays keeps the edges and the clear-air map (or one word per layer) in at most 64 KB: at the deepest 1 x 1
    column it accepts (bisection on host-side refusals) every ray matches the oracle bit for bit from every place that accepts
    the domain -- the bricked field with its clear-air map, the linear field, and the column record over a base profile, whose
    profile is what fills the hook's LDS at this depth; one layer more is refused on the host.  Probed: 8189 layers accepted, 8190 refused.  (The hook cannot trace the
    40 443-layer column of the launches' own limit: its 64 KB are its own limit, below theirs.)"""
    from tests.test_gpu_parity import _random_rays, make_oracle

    tab = _hg(0.85)
    rng = np.random.default_rng(5)

    def accepted(nz):
        g = _make(_column(nz, ssa=0.9), tab)
        try:
            g.trace_rays(np.array([[0.0, 0.0, 1.0]]), np.array([[50.0, 50.0, 0.1]]), np.array([[1, 1, 1]]))
            return True
        except I3RCError as e:
            assert "do not fit in LDS" in str(e), e
            return False
        finally:
            g.finalize_Integrator()

    lo, hi = 1000, 20_000
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    print(f"trace_rays: nz {lo} accepted, {hi} refused")
    d = _column(lo, ssa=0.9)
    o = make_oracle(oracle, d, [tab.inverse_table(9001)])
    n = 600
    dirs, pos, idx, target = _random_rays(rng, d, n, o)
    g = _make(d, tab)
    assert g.has_column_records()   # (a single column is its own base profile: column records over it, GRID_COLBASE)
    g.finalize_Integrator()
    for place in ("auto", "linear", "columns"):
        g = _make(d, tab)
        g.select_grid_place(place)
        tau, p2, i2, steps = g.trace_rays(dirs, pos, idx, target)
        for k in range(n):
            t, pp, ii, ss = o.trace(dirs[k], pos[k], idx[k], None if target[k] < 0 else float(target[k]))
            assert f32(t) == tau[k], (place, k, t, tau[k])
            assert np.array_equal(pp, p2[k]) and list(i2[k]) == ii and ss == steps[k], (place, k)
        g.finalize_Integrator()


def test_a_launch_beyond_a_compute_units_lds_is_refused_on_the_host():
    """Column records over a base profile keep the profile in LDS beside the edges.  A deep two-component column that plan_launch's
    edge check accepts (22 000 layers: edges and profile 176 KB): on the automatic place it now reads the field linearly and runs;
    with the column records asked for, launch's own check (160 KB - 256) refuses it before anything reaches the device, nothing is
    tallied, and the handle still runs afterwards.  A field of that depth beyond 4 MB reads its bricks instead, and equals the
    plainest launch."""
    d = _column(22_000, ncomp=2, ssa=0.9)
    g = _make(d, [_hg(0.85), _hg(0.0)], surfaceAlbedo=0.2)
    assert g.has_column_records()
    ok = _run(g, n=2001)
    assert g.last_plan()["place"] == 1 and ok["counters"]["photons"] == 2001, g.last_plan()
    g.select_grid_place("columns")
    with pytest.raises(I3RCError, match="more LDS than a compute unit has"):
        _run(g, n=2001)
    assert not g.fetch().any()
    g.select_grid_place("linear")
    again = _run(g, n=2001)
    _same(ok, again, 0, "after the refusal")
    g.finalize_Integrator()
    # a field of that depth beyond 4 MB: the automatic place reads it in bricks, as it would without the records
    d = _deep_clouds(20_500)
    g = _make(d, [_hg(0.85), _hg(0.0)], surfaceAlbedo=0.2)
    assert g.has_column_records()
    got = _run(g, n=2001)
    assert g.last_plan()["place"] == 2, g.last_plan()
    assert got["counters"]["scatterings"] > 0
    _plainest(g)
    _same(got, _run(g, n=2001), 0, "bricks against the plainest launch")
    g.finalize_Integrator()


def _deep_clouds(nz, nx=64):
    """nx x 1 columns of one cloud run each (column 0 clear) over a horizontally uniform gas: column records over a base profile"""
    ze = np.arange(nz + 1, dtype=f32)
    gas = np.broadcast_to(np.linspace(2e-5, 1e-5, nz, dtype=f32)[:, None, None], (nz, 1, nx)).copy()
    cloud = np.zeros((nz, 1, nx), f32)
    for c in range(1, nx):
        cloud[100 * c:100 * c + 50 * c, 0, c] = f32(0.01 * (1 + c % 5))
    return dict(xe=f32(10.0) * np.arange(nx + 1, dtype=f32), ye=np.array([0.0, 10.0], f32), ze=ze, ext=[cloud, gas],
                ssa=[np.full(cloud.shape, f32(0.9)), np.ones(gas.shape, f32)],
                pf=[(cloud > 0).astype(np.int32), np.ones(gas.shape, np.int32)])


# ---- 6. the absorbing flag ---------------------------------------------------------------------------------------------------------
def test_conservative_domain_with_empty_absorbing_cells_is_not_absorbing():
    """h->absorbing comes from the components the kernels can select in each cell.  A conservative gas + cloud domain whose gas --
    the FIRST component -- is zero in some cells and carries omega = 0 there: the gas is never selected in those cells (a deviate
    in [0, 1] is never below its cumulative fraction 0), so the domain tallies no volume absorption (plan: not absorbing, no volume
    tallies in LDS), gives fluxAbsorbed = volumeAbsorption = 0 exactly, and equals the same domain with omega = 1 in those cells --
    for any seed.  (Before the fix the flag was set from the albedo of every cell of every component: this domain was absorbing.)
    The same gas as the LAST component can be selected there -- by a deviate of exactly 1.0, which the kernels draw about once in
    2^25 -- so that domain is absorbing, and its fluxAbsorbed is the column sum of its volumeAbsorption."""
    from tools import cases

    c = cases.step_cloud(ssa=1.0, nlayers=8, ncolumns=16)
    gas = np.full_like(c["ext"], f32(2e-3))
    gas[:, :, ::3] = 0.0
    gas[3] = 0.0
    gas_pf = np.where(gas > 0, 1, 0).astype(np.int32)
    out = []
    for empty_ssa in (0.0, 1.0):
        s = np.where(gas > 0, f32(1.0), f32(empty_ssa)).astype(f32)
        d = dict(c, ext=[gas, c["ext"]], ssa=[s, c["ssa"]], pf=[gas_pf, c["pf"]])
        g = _make(d, [_hg(0.0), _hg(0.85)], surfaceAlbedo=0.3)
        r = _run(g)
        plan = g.last_plan()
        assert plan["absorbing"] == 0 and plan["ldsVolume"] == 0, (empty_ssa, plan)
        assert not r["fluxAbsorbed"].any() and not r["volumeAbsorption"].any()
        out.append(r)
        g.finalize_Integrator()
    assert out[0]["counters"]["scatterings"] > 0
    _same(out[0], out[1], 0, "omega of the empty cells")
    # the gas last: selectable with a deviate of 1.0 where the cloud's cumulative fraction is 1
    s = np.where(gas > 0, f32(1.0), f32(0.0)).astype(f32)
    g = _make(dict(c, ext=[c["ext"], gas], ssa=[c["ssa"], s], pf=[c["pf"], gas_pf]), [_hg(0.85), _hg(0.0)], surfaceAlbedo=0.3)
    r = _run(g)
    assert g.last_plan()["absorbing"] == 1, g.last_plan()
    lay = g.layout()
    ncol = g.nx * g.ny
    vol = r["raw"][lay.volumeAbsorption:lay.volumeAbsorption + g.nz * ncol].reshape(g.nz, ncol)
    col = np.zeros(ncol)
    for k in range(g.nz):   # (absorbed_columns' order of the float64 additions)
        col += vol[k]
    assert np.array_equal(r["raw"][lay.fluxAbsorbed:lay.fluxAbsorbed + ncol], col)
    g.finalize_Integrator()
