"""The launches whose decisions tests/golden/launch_plans.json records: small domains x parameters x knobs of the handle x kind of
launch, in the style of tests/kernel_matrix.py, on both sides of everything the host decides about a launch -- the place of the
extinction field, each LDS region at the last size that has it and the first that has not, the inverse table in LDS, the start
stores, the class of the problem and the kernel variant, the extra tallies, and the refusals.

tools/record_launch_plans.py runs every row as a real one-photon launch and writes down the plan and the kernel's name (or the
refusal's text); tests/test_launch_plan_cpu.py asks the host-only entries i3rc_hip_problem_facts / i3rc_hip_plan_launch for the same
rows and wants the same answers.  A row says everything both need: the domain (a spec, built by domain()), the parameters, the size of
the inverse tables, the knobs (kernel variant, grid place, partial sums in LDS), the kind of the launch and of the source."""
import numpy as np

f32 = np.float32

RAD1 = dict(intensityMus=[0.8], intensityPhis=[30.0], useRussianRouletteForIntensity=True, zetaMin=0.3)
RAD2 = dict(intensityMus=[0.9, 0.5], intensityPhis=[0.0, 120.0], useRussianRouletteForIntensity=True, zetaMin=0.3)
RAD8 = dict(intensityMus=[1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], intensityPhis=[0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0])
PARAMS = {
    "flux": dict(surfaceAlbedo=0.3),
    "rad1": dict(RAD1, surfaceAlbedo=0.3),
    "rad2": dict(RAD2, surfaceAlbedo=0.3),
    "rad8": dict(RAD8, surfaceAlbedo=0.3),
    "maxcs": dict(surfaceAlbedo=0.3, useRayTracing=False),
    "maxcs rad2": dict(RAD2, surfaceAlbedo=0.3, useRayTracing=False),
}
SOURCE = (0.7, 30.0)          # solar mu, azimuth
DEFAULT_INV = 9001            # steps of the inverse tables a handle makes for itself (host.DEFAULT_MIN_TABLE_SIZE)
SMALL_INV = 129


def directions(params):
    return len(PARAMS[params].get("intensityMus", ()))


# ---- domains ------------------------------------------------------------------------------------------------------------------------
def _hg(*gs):
    import i3rc_monte_carlo_model_amd as M

    return M.PhaseFunctionTable([M.henyey_greenstein(g, 32) for g in gs])


def _empty(nx, ny, nz):
    """optically empty: width * largest extinction below 1e-5"""
    ext = np.full((nz, ny, nx), f32(1e-9))
    return dict(xe=(f32(10.0) * np.arange(nx + 1)).astype(f32), ye=(f32(10.0) * np.arange(ny + 1)).astype(f32),
                ze=np.linspace(0.0, 100.0, nz + 1).astype(f32), ext=ext, ssa=np.full(ext.shape, f32(0.9)), pf=np.ones(ext.shape, np.int32))


def _tall(nx, ny, nz):
    """more layers than the bricked field's clear-air map counts, every cell the same"""
    ext = np.full((nz, ny, nx), f32(1e-5))
    return dict(xe=(f32(10.0) * np.arange(nx + 1)).astype(f32), ye=(f32(10.0) * np.arange(ny + 1)).astype(f32),
                ze=np.arange(nz + 1, dtype=f32), ext=ext, ssa=np.full(ext.shape, f32(0.9)), pf=np.ones(ext.shape, np.int32))


def _wide(n, nz=9, ncomp=1):
    """n x n columns of random cells, regular: beyond an XCD's L2 from n = 342 (nz = 9)"""
    rng = np.random.default_rng(2)
    ext = (rng.uniform(0.2, 1.0, (nz, n, n)) / 100.0).astype(f32)
    d = dict(xe=(f32(30.0) * np.arange(n + 1)).astype(f32), ye=(f32(30.0) * np.arange(n + 1)).astype(f32),
             ze=np.linspace(0.0, 300.0, nz + 1).astype(f32), ext=ext, ssa=np.full(ext.shape, f32(0.9)), pf=np.ones(ext.shape, np.int32))
    if ncomp == 2:
        d = dict(d, ext=[ext, f32(0.5) * ext], ssa=[d["ssa"], np.ones_like(d["ssa"])], pf=[d["pf"], d["pf"]])
    return d


def domain(spec):
    """(dict of the tools.cases form, list of phase-function tables, one per component) of a row's domain spec"""
    from tests import kernel_matrix as K
    from tests import test_gpu_limits as L

    kind, args = spec[0], spec[1:]
    if kind == "matrix":
        return K.DOMAINS[args[0]]()
    if kind == "lds_case":                       # the shapes of test_gpu_limits.LDS_CASES
        d = L.LDS_CASES[args[0]][0](args[1])
    elif kind == "box":                          # (nx, ny, nz, ssa, regular)
        d = L._box(args[0], args[1], args[2], ssa=args[3], regular=bool(args[4]))
    elif kind == "column":                       # (nz, ncomp)
        d = L._column(args[0], ncomp=args[1], ssa=0.9)
    elif kind == "deep_clouds":                  # (nz, nx)
        d = L._deep_clouds(args[0], nx=args[1])
    elif kind == "empty":
        d = _empty(*args)
    elif kind == "tall":
        d = _tall(*args)
    elif kind == "wide":
        d = _wide(*args)
    else:
        raise KeyError(spec)
    ncomp = len(d["ext"]) if isinstance(d["ext"], list) else 1
    return d, [_hg(0.85)] + [_hg(0.0)] * (ncomp - 1)


def surface(which):
    """a row's surface description: None, "one" (a single cell: reflects like surfaceAlbedo) or "grid" (2 x 2 cells)"""
    import i3rc_monte_carlo_model_amd as M

    if which == "one":
        return M.new_SurfaceDescription([0.25])
    if which == "grid":
        return M.new_SurfaceDescription(np.array([[0.1, 0.2], [0.3, 0.4]], f32), np.array([0.0, 1e4, 1e9], f32), np.array([0.0, 1e4, 1e9], f32))
    return None


def arrays(d):
    """what Integrator.__init__ hands i3rc_hip_create for a domain of the tools.cases form: (nx, ny, nz, ncomp, xe, ye, ze, total, cum, ssa, pf)"""
    import i3rc_monte_carlo_model_amd as M

    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    lists = [d[k] if isinstance(d[k], list) else [d[k]] for k in ("ext", "ssa", "pf")]
    hg = M.henyey_greenstein(0.85, 32)
    for i, (e, s, p) in enumerate(zip(*lists)):   # (a table of as many entries as the cells name: addOpticalComponent checks that)
        dom.addOpticalComponent(f"component {i + 1}", e, s, p, M.PhaseFunctionTable([hg] * max(1, int(np.max(p)))))
    total, cum, ssa, pfi, _ = dom.getOpticalPropertiesByComponent()
    one = f32(1.0)
    last = cum[-1]
    last[np.abs(last - one) <= np.spacing(one)] = one + np.spacing(one)   # (Integrator.__init__: r == 1 still selects the last component)
    nz, ny, nx = total.shape
    c = np.ascontiguousarray
    return (nx, ny, nz, cum.shape[0], c(dom.x, f32), c(dom.y, f32), c(dom.z, f32), c(total, f32), c(cum, f32), c(ssa, f32), c(pfi, np.int32))


# ---- the host-only entries on a row (no device) ---------------------------------------------------------------------------------------
KERNELS = {"auto": 0, "general": 1, "lane": 2, "ring": 3}           # host.Integrator.KERNELS
GRID_PLACES = {"auto": 0, "linear": 1, "bricks": 2, "columns": 3}   # host.Integrator.GRID_PLACES
SURFACE_CELLS = {None: (0, 0), "one": (1, 1), "grid": (2, 2)}


def facts(d, env=None):
    """i3rc_hip_problem_facts on a domain of the tools.cases form"""
    from i3rc_monte_carlo_model_amd import binding as B

    return B.problem_facts(*arrays(d), env=env)


def setup(params, entries, inv, kind="plain", kernel="auto", place="auto", lds_tallies=True, surface=None):
    """the words of binding.SETUP_NAMES a handle would be in after specifyParameters(**params) (a dict), set_tables with `inv` steps
    and `entries` entries of component 1, and its knobs"""
    nd = len(params.get("intensityMus", ()))
    nxs, nys = SURFACE_CELLS[surface]
    return dict(nDir=nd, inverseTables=1, forwardTables=int(nd > 0), inverseSteps=inv, inverseEntries=entries, useSurfaceBDRF=int(surface is not None),
                useRayTracing=int(params.get("useRayTracing", True)), surfaceNx=nxs, surfaceNy=nys, surfaceSet=int(surface is not None),
                extra={"level": 1, "track": 2}.get(kind, 0), kernelVariant=KERNELS[kernel], gridPlace=GRID_PLACES[place], ldsTalliesOn=int(lds_tallies))


def decide(row, env=None):
    """(kernel name, plan) or (refusal text, None) of a row, from i3rc_hip_problem_facts and i3rc_hip_plan_launch"""
    from i3rc_monte_carlo_model_amd import binding as B

    d, tabs = domain(row["domain"])
    s = setup(PARAMS[row["params"]], tabs[0].n_entries, row["inv"], row["kind"], row["kernel"], row["place"], row["lds_tallies"], row["surface"])
    return B.plan_launch(facts(d, env), s, stream=row["kind"], source=row["src"], fused_batches=int(row["kind"] == "fused"), env=env)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _row(rid, dom, params="flux", kind="plain", kernel="auto", place="auto", lds_tallies=True, inv=SMALL_INV, surface=None, src=0,
         refused=False):
    return dict(id=rid, domain=tuple(dom), params=params, kind=kind, kernel=kernel, place=place, lds_tallies=lds_tallies, inv=inv,
                surface=surface, src=src, refused=refused)


# the five LDS edges of test_gpu_limits.LDS_CASES: sizes around the pair its docstring names
EDGES = {"ldsTallies": 314, "ldsVolume": 261, "ldsIntensity": 84, "ldsGrid": 450, "tableInLds": 193}
EDGE_PARAMS = {"ldsIntensity": "rad2"}
# the track-length sums in LDS: 7 x 5 x k conservative cells, around the size at which the launch's allocation is full
TRACK_SIZES = (300, 380, 384, 385, 386, 390, 391, 392, 440, 455)


def _table():
    R = []
    M7 = ("step", "step_arrays", "step_records", "two", "three", "columns2", "colbase2")
    # 1. the matrix domains: classes x variants x kinds, on the automatic place (the field in LDS) ...
    for dom in M7:
        full = dom in ("step", "step_records", "two", "colbase2")
        for params in ("flux", "rad1", "rad2") if full else ("flux", "rad2"):
            for kernel in ("auto", "general", "lane", "ring") if full else ("auto",):
                R.append(_row(f"{dom}/{params}/{kernel}", ("matrix", dom), params, kernel=kernel))
            R.append(_row(f"{dom}/{params}/fused", ("matrix", dom), params, kind="fused"))
    # ... on every place that can be forced, plain and fused, with the default tables (the table form where it exists)
    for dom in M7:
        for place in ("linear", "bricks", "columns"):
            if place == "columns" and dom in ("two", "three"):
                continue                                     # (no column records: select_grid_place refuses)
            for kind in ("plain", "fused"):
                R.append(_row(f"{dom}/flux/{place}/{kind}", ("matrix", dom), "flux", kind=kind, place=place, inv=DEFAULT_INV))
            if dom in ("step", "step_records", "two", "colbase2"):
                R.append(_row(f"{dom}/rad2/{place}", ("matrix", dom), "rad2", place=place))
    for dom in ("step", "two", "colbase2"):
        R.append(_row(f"{dom}/flux/auto/default tables", ("matrix", dom), "flux", inv=DEFAULT_INV))
        R.append(_row(f"{dom}/flux/auto/default tables/fused", ("matrix", dom), "flux", kind="fused", inv=DEFAULT_INV))
    # 2. the LDS edges (default tables, as the handle makes them)
    for flag, k0 in EDGES.items():
        for k in range(k0 - 1, k0 + 3):
            R.append(_row(f"edge/{flag}/{k}", ("lds_case", flag, k), EDGE_PARAMS.get(flag, "flux"), inv=DEFAULT_INV))
    # ... the table form of fused launches (no start stores beside it) around its own edge, and with small tables
    for k in (307, 308):                                      # (the pair of sizes the table form of plain launches had before the start stores)
        R.append(_row(f"edge/tableInLds/{k}", ("lds_case", "tableInLds", k), "flux", inv=DEFAULT_INV))
    for k in (307, 308, 310, 311, 312, 313, 333, 338, 350):
        R.append(_row(f"edge/tableInLds fused/{k}", ("lds_case", "tableInLds", k), "flux", kind="fused", inv=DEFAULT_INV))
    for k in (307, 308, 350):
        R.append(_row(f"edge/tableInLds small tables/{k}", ("lds_case", "tableInLds", k), "flux"))
    # ... the same edges without partial sums in LDS
    for flag, k0 in EDGES.items():
        R.append(_row(f"edge/{flag}/{k0}/no lds tallies", ("lds_case", flag, k0), EDGE_PARAMS.get(flag, "flux"), lds_tallies=False, inv=DEFAULT_INV))
    R.append(_row("two/rad2/no lds tallies", ("matrix", "two"), "rad2", lds_tallies=False))
    R.append(_row("step/flux/fused/no lds tallies", ("matrix", "step"), "flux", kind="fused", lds_tallies=False))
    # 3. the automatic place beyond LDS: column records, the linear field, bricks beyond 4 MB
    for ncomp in (1, 2):
        for n in (341, 342):                                  # 9 layers of n x n cells: 4 186 116 and 4 210 704 bytes
            for params in ("flux", "rad2"):
                R.append(_row(f"wide/{n}/{ncomp}/{params}", ("wide", n, 9, ncomp), params, inv=DEFAULT_INV))
        R.append(_row(f"wide/342/{ncomp}/flux/fused", ("wide", 342, 9, ncomp), "flux", kind="fused", inv=DEFAULT_INV))
    R.append(_row("wide/342/1/flux/linear", ("wide", 342, 9, 1), "flux", place="linear", inv=DEFAULT_INV))
    R.append(_row("step 64 x 64/flux", ("box", 64, 64, 8, 0.9, 1), "flux", inv=DEFAULT_INV))
    # records over a base profile: kept while edges and profile fit, else the field as without them; forced, the launch's own check
    for nz in (20_000, 20_300, 20_500):
        R.append(_row(f"column 2/{nz}/auto", ("column", nz, 2), "flux"))
    R.append(_row("column 2/20300/columns", ("column", 20_300, 2), "flux", place="columns"))
    R.append(_row("column 2/20500/columns", ("column", 20_500, 2), "flux", place="columns", refused=True))
    R.append(_row("deep clouds/20500", ("deep_clouds", 20_500, 64), "flux"))
    R.append(_row("column 2/2000/replay", ("column", 2000, 2), "flux", kind="replay", src=1))
    # more than 65534 layers: the edge vectors alone are beyond a compute unit's LDS
    R.append(_row("tall/65535", ("tall", 6, 3, 65_535), "flux", refused=True))
    R.append(_row("column/40443", ("column", 40_443, 1), "flux"))
    R.append(_row("column/40444", ("column", 40_444, 1), "flux", refused=True))
    # 4. the start stores: on top of everything else, up to a compute unit's LDS -- beyond it the general flux kernel
    for nz in (30_000, 38_000, 38_800, 39_000, 39_200, 39_400, 39_600, 40_000):
        R.append(_row(f"column/{nz}", ("column", nz, 1), "flux"))
    # 5. the extra tallies (the general flux kernel), the track sums in LDS and just past it
    for dom in ("step", "two", "colbase2"):
        for kind in ("level", "track"):
            for place in ("auto", "linear", "bricks"):
                R.append(_row(f"{dom}/{kind}/{place}", ("matrix", dom), "flux", kind=kind, place=place))
    for k in TRACK_SIZES:
        R.append(_row(f"track/{k}", ("box", 7, 5, k, 1.0, 1), "flux", kind="track"))
    R.append(_row("track/380/no lds tallies", ("box", 7, 5, 380, 1.0, 1), "flux", kind="track", lds_tallies=False))
    R.append(_row("level/380", ("box", 7, 5, 380, 1.0, 1), "flux", kind="level"))
    # 6. surfaces, max cross-section, explicit photons, the replay build
    for dom in ("step", "two"):
        for surf in ("one", "grid"):
            for params in ("flux", "rad2"):
                R.append(_row(f"{dom}/{params}/surface {surf}", ("matrix", dom), params, surface=surf))
            R.append(_row(f"{dom}/flux/surface {surf}/fused", ("matrix", dom), "flux", kind="fused", surface=surf))
        for params in ("maxcs", "maxcs rad2"):
            R.append(_row(f"{dom}/{params}", ("matrix", dom), params))
        R.append(_row(f"{dom}/flux/explicit photons", ("matrix", dom), "flux", src=1))
        R.append(_row(f"{dom}/rad2/explicit photons", ("matrix", dom), "rad2", src=1))
        R.append(_row(f"{dom}/flux/replay", ("matrix", dom), "flux", kind="replay", src=1))
        R.append(_row(f"{dom}/rad2/replay", ("matrix", dom), "rad2", kind="replay", src=1))
    for params in ("maxcs", "maxcs rad2", "flux"):
        R.append(_row(f"empty/{params}", ("empty", 6, 4, 5), params))
    R.append(_row("empty/maxcs/fused", ("empty", 6, 4, 5), "maxcs", kind="fused"))
    R.append(_row("step/rad8", ("matrix", "step"), "rad8"))
    R.append(_row("two/rad8/fused", ("matrix", "two"), "rad8", kind="fused"))
    ids = [r["id"] for r in R]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return R


ROWS = _table()
