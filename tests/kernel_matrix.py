"""One recipe per production instantiation of photon_kernel: the checklist that tests/test_build_isa.py holds equal to the
instantiations the library compiles, and that tests/test_gpu_kernel_matrix.py runs on the device.

A recipe names its target exactly as i3rc_hip_last_kernel_name reports it (the form of tools/kernel_resources.demangle_photon_kernel)
and says how a caller reaches it: a small domain (DOMAINS), the parameters (PARAMS), the knobs of the handle -- the kernel variant
(set_tuning(kernel=...)), the place of the extinction field (select_grid_place), fused batches (set_batch_fusion(1)) -- and, where
nothing else reaches it, the environment of a process of its own (variables the library reads once per process).

Every domain absorbs somewhere (omega < 1) and every recipe has a reflecting surface; the radiance recipes use Iwabuchi's roulette,
and the one on the bricked field of each radiance family the hybrid tables with the contribution limit.  The domains read a cell's
albedo and table entry in every form the kernels know: kernel arguments (one component, shared values), plain arrays (one
component, entries not shared), 8-byte records (one component, neither shared), 16-byte records (two components) and 32-byte
records (three components); the field is read from LDS, linearly, in bricks, as column records and as column records over a
base profile."""
import numpy as np

f32 = np.float32

PLACES = ("GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE")
# select_grid_place for a target place: a small field sits in LDS on "auto"; records over a base profile are what "columns" reads
# from a field that has them
PLACE_KNOB = {"GRID_LDS": "auto", "GRID_GLOBAL": "linear", "GRID_BRICKS": "bricks", "GRID_COLUMNS": "columns", "GRID_COLBASE": "columns"}


# ---- domains: each (dict of the cases.* form, list of phase-function tables), small enough for the field to fit in LDS --------------
def _tables(*gs):
    import i3rc_monte_carlo_model_amd as M

    # (the first entry sharp enough for the hybrid tables' Gaussian splice to exist)
    return M.PhaseFunctionTable([M.henyey_greenstein(0.95, 299) if g == 0.95 else M.henyey_greenstein(g, 32) for g in gs])


def _step():
    """one component, every value shared: albedo and table entry travel in the kernel arguments (column records: one run per column)"""
    from tools import cases

    return cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)


def step():
    return _step(), [_tables(0.95)]


def step_arrays():
    """one component, one albedo, two table entries: the entries are read from their plain array"""
    d = _step()
    pf = np.ones_like(d["pf"])
    pf[:, :, 1::3] = 2
    pf[::2, :, 5::4] = 2
    return dict(d, pf=pf), [_tables(0.95, 0.6)]


def step_records():
    """one component, neither albedo nor entry shared: the 8-byte cell records"""
    d = _step()
    pf = np.ones_like(d["pf"])
    pf[1::2] = 2
    ssa = np.full_like(d["ssa"], f32(0.999))
    ssa[:, :, ::3] = f32(0.9)
    return dict(d, pf=pf, ssa=ssa), [_tables(0.95, 0.6)]


def two():
    """two components, regular grid (cloud + horizontally uniform gas): 16-byte records"""
    from tools import cases

    return cases.two_component(), [_tables(0.95, 0.6), _tables(0.0)]


def three():
    """three components (droplets + aerosol + gas): 32-byte records"""
    from tools import cases

    d = cases.two_component(seed=9, nx=7, ny=3, nz=9)
    aer = np.zeros_like(d["ext"][0])
    aer[:3] = f32(0.002)
    return dict(d, ext=[d["ext"][0], aer, d["ext"][1]], ssa=[d["ssa"][0], np.where(aer > 0, f32(0.92), f32(0)).astype(np.float32), d["ssa"][1]],
                pf=[d["pf"][0], (aer > 0).astype(np.int32), d["pf"][1]]), [_tables(0.95, 0.6), _tables(0.7), _tables(0.0)]


def columns2():
    """two components inside the same runs of an irregular grid of column clouds: column records (16-byte cell records)"""
    from tools import cases

    d = cases.column_clouds()
    aer = (d["ext"] * f32(0.25)).astype(np.float32)
    ssa2 = np.where(aer > 0, f32(0.8), f32(0)).astype(np.float32)
    return dict(d, ext=[d["ext"], aer], ssa=[d["ssa"], ssa2], pf=[d["pf"], (aer > 0).astype(np.int32)]), [_tables(0.95), _tables(0.6)]


def colbase2():
    """column clouds plus a horizontally uniform gas: column records over a base profile"""
    from tools import cases

    d = cases.column_clouds()
    nz = d["ext"].shape[0]
    gas = np.ascontiguousarray(np.broadcast_to(np.linspace(0.003, 0.001, nz, dtype=np.float32)[:, None, None], d["ext"].shape), np.float32)
    return dict(d, ext=[d["ext"], gas], ssa=[d["ssa"], np.full_like(gas, f32(0.6))], pf=[d["pf"], np.ones(gas.shape, np.int32)]), \
        [_tables(0.95), _tables(0.0)]


DOMAINS = {f.__name__: f for f in (step, step_arrays, step_records, two, three, columns2, colbase2)}

_RRI = dict(useRussianRouletteForIntensity=True, zetaMin=0.3)
_HYBRID = dict(useHybridPhaseFunsForIntenCalcs=True, hybridPhaseFunWidth=7.0, numOrdersOrigPhaseFunIntenCalcs=1,
               limitIntensityContributions=True, maxIntensityContribution=0.5)
PARAMS = {
    "flux": dict(surfaceAlbedo=0.3),
    "ring": dict(_RRI, surfaceAlbedo=0.2, intensityMus=[1.0, 0.5], intensityPhis=[0.0, 120.0]),
    "ring hybrid": dict(_RRI, **_HYBRID, surfaceAlbedo=0.2, intensityMus=[0.9, 0.4], intensityPhis=[10.0, 200.0]),
    "direct": dict(_RRI, surfaceAlbedo=0.2, intensityMus=[0.8], intensityPhis=[30.0]),
    "direct hybrid": dict(_RRI, **_HYBRID, surfaceAlbedo=0.2, intensityMus=[1.0], intensityPhis=[0.0]),
}
SOURCE = (0.7, 25.0)   # solar mu, azimuth


def directions(params):
    return len(PARAMS[params].get("intensityMus", ()))


def _name(rng, intensity, general, place, tbl=False, direct=False, wide=False):
    return (f"photon_kernel<{rng}, {'true' if intensity else 'false'}, {'true' if general else 'false'}, {place}"
            f"{', table in LDS' if tbl else ''}{', one direction' if direct else ''}{', wide' if wide else ''}>")


def _recipe(rng, intensity, general, place, domain, params, kernel="auto", tbl=False, direct=False, wide=False, env=None):
    return dict(target=_name(rng, intensity, general, place, tbl, direct, wide), domain=domain, params=params, kernel=kernel,
                place=PLACE_KNOB[place], fused=rng == "PhiloxBatchStream", env=dict(env or {}))


def _table():
    R = []
    S, B = "PhiloxStream", "PhiloxBatchStream"
    # ---- plain launches (launch()) --------------------------------------------------------------------------------------------------
    # general kernels: set_tuning(kernel="general")
    for place, dom in zip(PLACES, ("two", "three", "step_records", "columns2", "colbase2")):
        R.append(_recipe(S, False, True, place, dom, "flux", kernel="general"))
    for place, dom, par in zip(PLACES, ("step_arrays", "two", "three", "step", "colbase2"), ("ring", "ring", "ring hybrid", "ring", "ring")):
        R.append(_recipe(S, True, True, place, dom, par, kernel="general"))
    for place, dom, par in zip(PLACES, ("three", "step_records", "two", "columns2", "colbase2"), ("direct", "direct", "direct hybrid", "direct", "direct")):
        R.append(_recipe(S, True, True, place, dom, par, kernel="general", direct=True))
    # specialised kernels (the common class: one component, regular grid); flux without the table in LDS: set_tuning(kernel="lane")
    for place, dom in zip(PLACES[:4], ("step_records", "step", "step_arrays", "step_records")):
        R.append(_recipe(S, False, False, place, dom, "flux", kernel="lane"))
    for place, dom, par in zip(PLACES[:4], ("step", "step_records", "step_arrays", "step_records"), ("ring", "ring", "ring hybrid", "ring")):
        R.append(_recipe(S, True, False, place, dom, par))
    for place, dom, par in zip(PLACES[:4], ("step_arrays", "step", "step_records", "step"), ("direct", "direct", "direct hybrid", "direct")):
        R.append(_recipe(S, True, False, place, dom, par, direct=True))
    # ... with the inverse table in LDS (one table entry); on a bricked field only where I3RC_TABLE_LDS_PLACES has bit 2 set
    for place in PLACES[:4]:
        R.append(_recipe(S, False, False, place, "step", "flux", tbl=True, env={"I3RC_TABLE_LDS_PLACES": "15"} if place == "GRID_BRICKS" else None))
    # several components / irregular grids (the widened class), radiance
    for place, dom, par in zip(PLACES, ("two", "three", "two", "columns2", "colbase2"), ("ring", "ring", "ring hybrid", "ring", "ring")):
        R.append(_recipe(S, True, False, place, dom, par, wide=True))
    for place, dom, par in zip(PLACES, ("three", "two", "three", "columns2", "colbase2"), ("direct", "direct", "direct hybrid", "direct", "direct")):
        R.append(_recipe(S, True, False, place, dom, par, direct=True, wide=True))
    # ---- fused batches (launch_fused_group): set_batch_fusion(1) -------------------------------------------------------------------
    # flux without the table in LDS: two table entries that the cells do not share (a bricked field never has it in LDS)
    for place, dom in zip(PLACES[:4], ("step_records", "step_arrays", "step", "step_records")):
        R.append(_recipe(B, False, False, place, dom, "flux"))
    for place in ("GRID_LDS", "GRID_GLOBAL", "GRID_COLUMNS"):
        R.append(_recipe(B, False, False, place, "step", "flux", tbl=True))
    for place, dom, par in zip(PLACES[:4], ("step", "step_arrays", "step_records", "step"), ("ring", "ring", "ring hybrid", "ring")):
        R.append(_recipe(B, True, False, place, dom, par))
    for place, dom, par in zip(PLACES[:4], ("step_records", "step", "step_arrays", "step_records"), ("direct", "direct", "direct hybrid", "direct")):
        R.append(_recipe(B, True, False, place, dom, par, direct=True))
    for place, dom in zip(PLACES, ("two", "three", "two", "columns2", "colbase2")):
        R.append(_recipe(B, False, False, place, dom, "flux", wide=True))
    for place, dom, par in zip(PLACES, ("three", "two", "three", "columns2", "colbase2"), ("ring", "ring", "ring hybrid", "ring", "ring")):
        R.append(_recipe(B, True, False, place, dom, par, wide=True))
    for place, dom, par in zip(PLACES, ("two", "three", "two", "columns2", "colbase2"), ("direct", "direct", "direct hybrid", "direct", "direct")):
        R.append(_recipe(B, True, False, place, dom, par, direct=True, wide=True))
    return R


RECIPES = _table()

# Production instantiations that no recipe reaches, with the reason.  Empty: an instantiation that neither the public API nor a
# documented environment switch reaches is taken out of the dispatch tables instead.
UNREACHABLE = {}
