"""Path-length moments of local-estimate radiances, the parts that need no GPU.

  symbols         the three entry points are declared, exported and bound; the kind is 5 and the stream 7
  layout          where the block's two fields lie and how long the buffer is, for three grids and nDir 1 and 3:
                  tests/radiance_path_main.cpp -- a host C++17 program over csrc/tally_block.hpp alone -- against the offsets restated
                  here; every other kind answers what it answered before the kind existed, and "off" is the layout without a block
  normalisation   random raw blocks through the header's normalised_extra_value against the radiance's rule restated in float64 numpy
                  (computeRadiativeTransfer :353-367, :385-388: the sum over the components divided by the photons per column, rounded
                  once to real(4)), bit for bit, on regular and irregular grids
  plan            stream kind 7 names a PhiloxRadiancePathStream ... true, true kernel at every place the general radiance kernel has,
                  with that kernel's plan; what the plan can see of the refusals -- no directions, max cross-section, a fused or a
                  replay launch -- is refused in words; kinds 0 ... 6 answer what they did
  ISA             exactly five kernels, none with scratch or a spilled vector register"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i3rc-monte-carlo-model_amd", "csrc")
NUM_COUNTERS, CNT_PHOTONS = 16, 0    # include/i3rc_hip.h
NEW_SYMBOLS = ("i3rc_hip_set_radiance_path_lengths", "i3rc_hip_get_radiance_path_length_layout", "i3rc_hip_normalise_radiance_path_lengths")
PLACES = ("GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE")
HEADER_WORDS = 50
HISTOGRAM_BINS = 7                   # (what the host program lays the path histogram out with)

GRIDS = {
    "1 x 1 x 4": dict(xe=[0.0, 500.0], ye=[0.0, 500.0], ze=[0.0, 0.25, 0.5, 0.75, 1.0], regular=1, ncomp=1),
    "3 x 2 x 2 irregular": dict(xe=[0.0, 10.0, 25.0, 31.0], ye=[-3.0, 4.5, 9.0], ze=[0.0, 0.3, 2.0], regular=0, ncomp=2),
    "8 x 4 x 6": dict(xe=list(62.5 * np.arange(9)), ye=list(125.0 * np.arange(5)), ze=[0.0, 30.0, 80.0, 120.0, 170.0, 210.0, 250.0], regular=1, ncomp=3),
}
CASES = [(name, nd) for name in GRIDS for nd in (1, 3)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("radiance_paths") / "radiance_path_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "radiance_path_main.cpp")])
    return str(exe)


def parent_layout(nx, ny, nz, ncomp, ndir):
    """i3rc_tally_layout as it was before the kind existed: the fields one behind the other, the counters last"""
    ncol = nx * ny
    counters = 3 * ncol + ncol * nz + (ncomp + 1) * ndir * ncol + (ncomp + 1) * ndir
    return dict(intensity=3 * ncol + ncol * nz, counters=counters, total=counters + NUM_COUNTERS)


def restated_layout(nx, ny, nz, ncomp, ndir):
    """... and with the radiance path block behind the counters: two fields of nDir nx ny words"""
    p = parent_layout(nx, ny, nz, ncomp, ndir)
    block = p["total"]
    return dict(p, radiancePath1=block, radiancePath2=block + ndir * nx * ny, block=block, total=block + 2 * ndir * nx * ny)


def run(program, g, ndir, tmp_path, seed=20251021):
    nx, ny, nz = len(g["xe"]) - 1, len(g["ye"]) - 1, len(g["ze"]) - 1
    lay = restated_layout(nx, ny, nz, g["ncomp"], ndir)
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.5, 5e4, lay["total"])
    raw[lay["counters"]:lay["counters"] + NUM_COUNTERS] = rng.integers(1, 1000, NUM_COUNTERS)
    raw[lay["counters"] + CNT_PHOTONS] = 20001.0
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nx, ny, nz, g["regular"], g["ncomp"], ndir], np.int64).tobytes())
        for k in ("xe", "ye", "ze"):
            f.write(np.float32(g[k]).tobytes())
        f.write(raw.tobytes())
    subprocess.check_call([program, str(src), str(dst)])
    header = np.fromfile(dst, np.int64, HEADER_WORDS).tolist()
    return lay, raw, header, np.fromfile(dst, np.float32, offset=8 * HEADER_WORDS)


def test_symbols_are_exported_and_bound_and_the_numbers_are_5_and_7():
    lib = M.binding.load()
    header = open(os.path.join(ROOT, "include", "i3rc_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in M.binding.SYMBOLS, name
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name
    assert M.binding.STREAM_KINDS["radiance_path"] == 7 and M.binding.EXTRA_KINDS["radiance_paths"] == 5
    # (and no earlier number has moved)
    assert M.binding.STREAM_KINDS == {"plain": 0, "fused": 1, "replay": 2, "level": 3, "track": 4, "path": 5, "bins": 6, "radiance_path": 7}
    assert M.binding.EXTRA_KINDS == {"none": 0, "levels": 1, "tracks": 2, "paths": 3, "bins": 4, "radiance_paths": 5}


@pytest.mark.parametrize("name,ndir", CASES)
def test_layout_of_the_block(program, name, ndir, tmp_path):
    g = GRIDS[name]
    nx, ny, nz = len(g["xe"]) - 1, len(g["ye"]) - 1, len(g["ze"]) - 1
    ncol = nx * ny
    lay, _, header, _ = run(program, g, ndir, tmp_path)
    got = dict(zip(("radiancePath1", "radiancePath2", "block", "counters", "total"), header[:5]))
    assert got == {k: lay[k] for k in got}, (got, lay)
    # every other kind: no radiance path offsets, and the offsets and total it had before the kind existed
    p = parent_layout(nx, ny, nz, g["ncomp"], ndir)
    block = p["total"]
    want = {
        "none": [-1, -1, -1, -1, -1, -1, -1, -1, p["total"]],                                  # (= the kind switched off)
        "levels": [-1, -1, block, block + (nz + 1) * ncol, -1, -1, -1, -1, block + 2 * (nz + 1) * ncol],
        "tracks": [-1, -1, -1, -1, -1, -1, -1, -1, block + nz * ncol],
        "paths": [-1, -1, -1, -1, block, block + ncol, block + 2 * ncol, block + 3 * ncol, block + 4 * ncol],
        "bins": [-1, -1, -1, -1, -1, -1, -1, -1, block + 4 * (HISTOGRAM_BINS + 1)],
    }
    for k, kind in enumerate(want):
        assert header[5 + 9 * k:14 + 9 * k] == want[kind], (kind, header[5 + 9 * k:14 + 9 * k], want[kind])


@pytest.mark.parametrize("name,ndir", CASES)
def test_normalisation_is_the_rule_of_the_radiance_bit_for_bit(program, name, ndir, tmp_path):
    g = GRIDS[name]
    lay, raw, _, got = run(program, g, ndir, tmp_path)
    xe, ye = (np.float64(np.float32(g[k])) for k in ("xe", "ye"))
    nx, ny = len(xe) - 1, len(ye) - 1
    ncol = nx * ny
    n_phot = raw[lay["counters"] + CNT_PHOTONS]
    if g["regular"]:                                                              # :355-356
        per_col = np.full((ny, nx), n_phot / float(nx * ny))
    else:                                                                         # :358-366
        per_col = ((ye[1:] - ye[:-1])[:, None] * (xe[1:] - xe[:-1])[None, :]) / ((xe[-1] - xe[0]) * (ye[-1] - ye[0])) * n_phot
    by_comp = raw[lay["intensity"]:lay["intensity"] + (g["ncomp"] + 1) * ndir * ncol].reshape(g["ncomp"] + 1, ndir, ny, nx)
    tot = np.zeros((ndir, ny, nx))
    for j in range(g["ncomp"] + 1):                                               # (the header's order of additions: component after component)
        tot = tot + by_comp[j]
    want = [np.float32(tot / per_col[None])]
    for at in (lay["radiancePath1"], lay["radiancePath2"]):
        want.append(np.float32(raw[at:at + ndir * ncol].reshape(ndir, ny, nx) / per_col[None]))
    want = np.concatenate([w.ravel() for w in want])
    assert got.shape == want.shape and np.all(np.isfinite(want)) and np.all(want > 0)
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, (name, ndir, differ[:8], got[differ[:8]], want[differ[:8]])


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def _rows():
    from tests import plan_sweep as S

    return [S._row(f"{dom}/rad2/{place}", ("matrix", dom), "rad2", kernel="general", place=place)
            for dom, place in (("step", "auto"), ("step", "linear"), ("two", "bricks"), ("columns2", "columns"), ("colbase2", "columns"),
                               ("two", "auto"), ("step_records", "bricks"))]


def _setups(row, **over):
    from tests import plan_sweep as S

    d, tabs = S.domain(row["domain"])
    plain = S.setup(S.PARAMS[row["params"]], tabs[0].n_entries, row["inv"], "plain", row["kernel"], row["place"], row["lds_tallies"], row["surface"])
    return S.facts(d), dict(plain, **over), dict(plain, extra=M.binding.EXTRA_KINDS["radiance_paths"], **over)


def test_kind_7_names_the_radiance_path_kernel_at_every_place_of_the_general_radiance_kernel():
    from i3rc_monte_carlo_model_amd import binding as B

    places = set()
    for row in _rows():
        facts, plain, paths = _setups(row)
        name_g, plan_g = B.plan_launch(facts, plain, stream="plain", source=row["src"])
        name_p, plan_p = B.plan_launch(facts, paths, stream="radiance_path", source=row["src"])
        assert plan_g is not None and plan_p is not None, (row["id"], name_g, name_p)
        assert name_g.startswith("photon_kernel<PhiloxStream, true, true, GRID_"), name_g
        assert name_p == name_g.replace("PhiloxStream", "PhiloxRadiancePathStream"), (name_g, name_p)
        assert plan_p == plan_g, (row["id"], plan_p, plan_g)                     # (the ring kernels' carve-up, no start store, 256 threads)
        assert plan_p["rayQueueCap"] == 64 and plan_p["startStoreBytes"] == 0 and plan_p["threads"] == 256, plan_p
        places.add(name_p.split(", ")[-1])
    assert places == {p + ">" for p in PLACES}, places


def test_kind_7_has_no_one_direction_form_and_takes_any_class_of_problem():
    """one direction, the automatic kernel choice, a gridded surface, explicit photons: always the general radiance kernel of the tag"""
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    for row in (S._row("step/rad1", ("matrix", "step"), "rad1"), S._row("two/rad8", ("matrix", "two"), "rad8"),
                S._row("step/rad2/grid", ("matrix", "step"), "rad2", surface="grid"), S._row("two/rad2/explicit", ("matrix", "two"), "rad2", src=1)):
        facts, _, paths = _setups(row)
        name, plan = B.plan_launch(facts, paths, stream="radiance_path", source=row["src"])
        assert plan is not None and name == "photon_kernel<PhiloxRadiancePathStream, true, true, GRID_LDS>", (row["id"], name)
        assert plan["rayQueueCap"] == 64, plan


def test_the_plan_refuses_what_it_can_see():
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    row = _rows()[0]
    facts, _, paths = _setups(row)
    text, plan = B.plan_launch(facts, dict(paths, nDir=0, forwardTables=0), stream="radiance_path")
    assert plan is None and "radiance path lengths are tallied by radiance launches only; no radiance direction is set (nDir = 0)" in text, text
    text, plan = B.plan_launch(facts, dict(paths, useRayTracing=0), stream="radiance_path")
    assert plan is None and "radiance path lengths need ray tracing; max cross-section is in use (useRayTracing = 0)" in text, text
    text, plan = B.plan_launch(facts, paths, stream="fused", fused_batches=4)
    assert plan is None and "radiance path lengths have no batch statistics yet" in text and "fused or announced batches cannot give them" in text, text
    text, plan = B.plan_launch(facts, paths, stream="replay", source=1)
    assert plan is None and "the replay stream cannot give them" in text, text
    # (max cross-section on an optically empty domain is traced: planned)
    d, tabs = S.domain(("empty", 6, 4, 5))
    empty = dict(S.setup(S.PARAMS["maxcs rad2"], tabs[0].n_entries, S.SMALL_INV), extra=M.binding.EXTRA_KINDS["radiance_paths"])
    name, plan = B.plan_launch(S.facts(d), empty, stream="radiance_path")
    assert plan is not None and "PhiloxRadiancePathStream, true, true" in name, name
    # an incomplete problem is refused in the words every launch hears
    text, plan = B.plan_launch(facts, dict(paths, forwardTables=0), stream="radiance_path")
    assert plan is None and "forward phase function table missing" in text, text


def test_kinds_0_to_6_answer_what_they_did_and_8_is_no_kind():
    """the recorded decisions (tests/golden/launch_plans.json, held by tests/test_launch_plan_cpu.py row by row) for one row of each
    recorded kind, and the path kinds against the level plan as their own tests hold them"""
    import ctypes as C
    import json

    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
        golden = json.load(f)["rows"]
    seen = set()
    for row in S.ROWS:
        if row["kind"] in seen or row["refused"]:
            continue
        seen.add(row["kind"])
        name, plan = S.decide(row)
        rec = golden[row["id"]] if isinstance(golden, dict) else next(r for r in golden if r["id"] == row["id"])
        assert name == rec["name"], (row["id"], name, rec)
    assert seen == {"plain", "fused", "replay", "level", "track"}, seen
    d, tabs = S.domain(("matrix", "step"))
    level = S.setup(S.PARAMS["flux"], tabs[0].n_entries, S.SMALL_INV, "level")
    name_l, plan_l = B.plan_launch(S.facts(d), level, stream="level")
    for stream, extra, tag, bins in (("path", 3, "PhiloxPathStream", 0), ("bins", 4, "PhiloxBinStream", 5)):
        name, plan = B.plan_launch(S.facts(d), dict(level, extra=extra), stream=stream, path_bins=bins)
        assert name == name_l.replace("PhiloxLevelStream", tag), (name, name_l)
        assert {k: plan[k] for k in plan_l if k != "ldsBytes"} == {k: plan_l[k] for k in plan_l if k != "ldsBytes"}, (stream, plan, plan_l)
    # stream kind 8: bad arguments (2), as 7 was
    facts = S.facts(d)
    out, text = (C.c_int32 * 20)(), C.create_string_buffer(512)
    rc = B.load().i3rc_hip_plan_launch((C.c_int32 * len(B.FACT_NAMES))(*[int(facts[k]) for k in B.FACT_NAMES]),
                                       (C.c_int32 * len(B.SETUP_NAMES))(*[int(level[k]) for k in B.SETUP_NAMES]), None,
                                       (C.c_int32 * 4)(8, 0, 0, 0), out, 16, text, len(text))
    assert rc == 2


def test_the_solver_s_path_moments_are_the_recorded_ones():
    """the reference of tests/test_gpu_radiance_path_lengths.py on its own: <L> / H and <L^2> / H^2 of the four slabs from the
    adding-doubling solver's derivatives in an absorber (n = 32), the two steps apart by what a third-moment term makes them, and the
    sanity case -- nearly all surface light -- near 1 / mu0 + 1 / mu = 3 and 4"""
    from tests.test_gpu_radiance_path_lengths import SLAB_CASES, solver_path_moments

    recorded = {(1.0, 1.0, 0.0): ((2.6280, 3.4003), (11.682, 18.254)), (1.0, 0.9, 0.5): ((3.2514, 3.9910), (12.494, 19.451)),
                (10.0, 1.0, 0.5): ((2.8521, 2.2915), (13.755, 10.379)), (0.1, 1.0, 0.5): ((3.1435, 4.1781), (11.816, 20.274))}
    assert set(SLAB_CASES) == set(recorded)
    for case, (l1, l2) in recorded.items():
        i0, r1, r2, s1, s2 = solver_path_moments(*case)
        assert np.abs(r1 / i0 / np.array(l1) - 1.0).max() < 3e-5, (case, (r1 / i0).tolist(), l1)
        assert np.abs(r2 / i0 / np.array(l2) - 1.0).max() < 5e-5, (case, (r2 / i0).tolist(), l2)
        assert (s1 / r1 < 1e-4).all() and (s2 / r2 < 1e-3).all(), (case, (s1 / r1).tolist(), (s2 / r2).tolist())
    i0, r1, _, _, _ = solver_path_moments(0.1, 1.0, 0.5)
    assert np.abs(r1 / i0 / np.array([3.0, 4.0]) - 1.0).max() < 0.05


def test_radiance_path_kernels_keep_their_state_in_registers():
    """exactly the five instantiations of the general radiance kernel, and as tests/test_build_isa.py asks of the production kernels:
    no spilled vector register, no scratch -- with the float64 path in two more registers of every lane and no ray registers"""
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources

    rows = [r for r in resources() if "PhiloxRadiancePathStream" in r["name"]]
    assert sorted(r["name"] for r in rows) == sorted(f"photon_kernel<PhiloxRadiancePathStream, true, true, {p}>" for p in PLACES), [r["name"] for r in rows]
    for r in rows:
        print(r["name"], "VGPRs", r["VGPRs"], "SGPR spills", r["SGPRs Spill"], "occupancy", r["Occupancy [waves/SIMD]"])
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (r["name"], r["VGPRs Spill"], r["ScratchSize [bytes/lane]"])
        assert r["Occupancy [waves/SIMD]"] >= 3, r
