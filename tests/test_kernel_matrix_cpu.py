"""The kernel matrix (tests/kernel_matrix.py) is a checklist: one recipe per production instantiation of photon_kernel, no more and no
fewer.  No GPU needed -- hipcc cross-compiles, and the domains' column records are made by host code."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import kernel_matrix as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def production_names():
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources

    return [r["name"] for r in resources() if r["name"].startswith(("photon_kernel<PhiloxStream,", "photon_kernel<PhiloxBatchStream,"))]


def test_every_production_instantiation_has_exactly_one_recipe(production_names):
    """Adding a dispatch-table entry (an instantiation) without a recipe, or a recipe for a kernel that is not compiled, fails here."""
    targets = [r["target"] for r in K.RECIPES]
    assert len(targets) == len(set(targets)), sorted(t for t in targets if targets.count(t) > 1)
    assert len(production_names) == len(set(production_names)), production_names
    assert not set(K.UNREACHABLE) & set(targets), set(K.UNREACHABLE) & set(targets)
    compiled, listed = set(production_names), set(targets) | set(K.UNREACHABLE)
    assert compiled == listed, ("compiled without a recipe", sorted(compiled - listed), "recipes without a kernel", sorted(listed - compiled))
    assert K.UNREACHABLE == {}, K.UNREACHABLE


def _host_view(domain):
    """(total extinction, component arrays) as new_Integrator hands them to the library"""
    import i3rc_monte_carlo_model_amd as M

    d, tabs = K.DOMAINS[domain]()
    dom = M.new_Domain(d["xe"], d["ye"], d["ze"])
    ext = d["ext"] if isinstance(d["ext"], list) else [d["ext"]]
    ssa = d["ssa"] if isinstance(d["ssa"], list) else [d["ssa"]]
    pf = d["pf"] if isinstance(d["pf"], list) else [d["pf"]]
    for i, (e, s, p, t) in enumerate(zip(ext, ssa, pf, tabs)):
        dom.addOpticalComponent(f"component {i + 1}", e, s, p, t)
    total = dom.getOpticalPropertiesByComponent()[0]
    return d, np.ascontiguousarray(total, np.float32), ext, ssa, pf


@pytest.mark.parametrize("domain", sorted(K.DOMAINS))
def test_each_domain_has_what_its_recipes_need(domain):
    """A recipe's domain must be able to reach its target: column records (with or without a base profile) where the target reads
    them, one component on a regular grid for the specialised kernels, several components or an irregular grid for the widened
    class; and every domain absorbs somewhere."""
    import i3rc_monte_carlo_model_amd as M

    lib = M.binding.load()
    d, total, ext, ssa, pf = _host_view(domain)
    nz, ny, nx = total.shape
    rec = np.zeros(2 * nx * ny, np.uint32)
    base = np.zeros(nz, np.float32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    plain = lib.i3rc_hip_column_records(nx, ny, nz, total.ctypes.data_as(fp), rec.ctypes.data_as(up)) == 1
    over_base = not plain and lib.i3rc_hip_column_records_base(nx, ny, nz, total.ctypes.data_as(fp), rec.ctypes.data_as(up), base.ctypes.data_as(fp)) == 1
    regular = all(np.allclose(np.diff(e), np.diff(e)[0], rtol=1e-6, atol=0) for e in (d["xe"], d["ye"]))
    assert any(((s < 1) & (e > 0)).any() for e, s in zip(ext, ssa)), domain
    for r in K.RECIPES:
        if r["domain"] != domain:
            continue
        t = r["target"]
        if "GRID_COLBASE" in t:
            assert over_base and len(ext) > 1, (domain, t)
        elif "GRID_COLUMNS" in t:
            assert plain, (domain, t)
        if ", false, GRID" in t and "wide" not in t:   # specialised kernels: the common class
            assert len(ext) == 1 and regular, (domain, t)
        if "wide" in t:
            assert len(ext) > 1 or not regular, (domain, t)
        if "table in LDS" in t:   # one table entry, or one that every cell shares
            assert len(ext) == 1 and len(np.unique(pf[0][ext[0] > 0])) == 1, (domain, t)
        elif r["fused"] and ", false, false" in t and "wide" not in t and "GRID_BRICKS" not in t:
            assert len(np.unique(pf[0][ext[0] > 0])) > 1, (domain, t)   # (fused flux keeps the table in LDS wherever it can)
        assert "surfaceAlbedo" in K.PARAMS[r["params"]] and K.PARAMS[r["params"]]["surfaceAlbedo"] > 0, t
        if K.directions(r["params"]):
            assert K.PARAMS[r["params"]].get("useRussianRouletteForIntensity"), t
        assert (K.directions(r["params"]) == 1) == ("one direction" in t), t
        assert (K.directions(r["params"]) > 0) == t.startswith(("photon_kernel<PhiloxStream, true", "photon_kernel<PhiloxBatchStream, true")), t


def test_cell_forms_and_hybrid_tables_are_covered():
    """one, two and three components (kernel arguments, plain arrays, 8-, 16- and 32-byte records), and hybrid tables with the
    contribution limit in every radiance family"""
    ncomp = {name: len(K.DOMAINS[name]()[0]["ext"]) if isinstance(K.DOMAINS[name]()[0]["ext"], list) else 1 for name in K.DOMAINS}
    used = {r["domain"] for r in K.RECIPES}
    assert used == set(K.DOMAINS)
    assert {ncomp[u] for u in used} == {1, 2, 3}
    assert {"step", "step_arrays", "step_records"} <= used
    families = {}
    for r in K.RECIPES:
        t = r["target"]
        if K.directions(r["params"]) == 0:
            continue
        fam = (t.split(",")[0], ", true, GRID" in t, "one direction" in t, "wide" in t)
        families.setdefault(fam, []).append("hybrid" in r["params"])
    assert len(families) == 10, families
    assert all(any(v) for v in families.values()), families
