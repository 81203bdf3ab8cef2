"""Where a launch is decided (csrc/launch_plan.hpp), asked through the host-only entries i3rc_hip_problem_facts and
i3rc_hip_plan_launch: no device.  The statement of what the decisions are is tests/golden/launch_plans.json -- real one-photon
launches of every row of tests/plan_sweep.py, recorded by tools/record_launch_plans.py at the commit the file names, BEFORE the
decisions moved into one function -- plus tests/kernel_matrix.py's recipes; the facts of a field are asserted on small arrays."""
import json
import os

import numpy as np
import pytest

from i3rc_monte_carlo_model_amd import binding as B
from tests import kernel_matrix as K
from tests import plan_sweep as S

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as _f:
    GOLDEN = json.load(_f)
CHUNK = B.PLAN_NAMES.index("chunk")        # (needs the device: the entry reports 0)


def _words(plan):
    return [plan[k] for i, k in enumerate(B.PLAN_NAMES) if i != CHUNK]


def test_golden_covers_the_sweep():
    assert GOLDEN["plan_names"] == B.PLAN_NAMES
    assert len(GOLDEN["commit"]) == 40
    assert sorted(GOLDEN["rows"]) == sorted(r["id"] for r in S.ROWS)
    assert 150 <= len(S.ROWS) <= 260
    refused = [r["id"] for r in S.ROWS if "refused" in GOLDEN["rows"][r["id"]]]
    assert sorted(refused) == sorted(r["id"] for r in S.ROWS if r["refused"]) and len(refused) >= 3


@pytest.mark.parametrize("row", S.ROWS, ids=[r["id"] for r in S.ROWS])
def test_decision_is_the_recorded_launch(row):
    """facts of the row's arrays, then the decision: exactly the recorded kernel name and plan words, or the recorded refusal"""
    want = GOLDEN["rows"][row["id"]]
    text, plan = S.decide(row)
    if "refused" in want:
        assert plan is None and text == want["refused"], (text, plan)
    else:
        assert plan is not None, text
        assert text == want["name"]
        assert _words(plan) == [v for i, v in enumerate(want["plan"]) if i != CHUNK], (plan, want["plan"])


@pytest.mark.parametrize("recipe", K.RECIPES, ids=[f"{r['target'].replace('photon_kernel', '')}{' env' if r['env'] else ''}" for r in K.RECIPES])
def test_kernel_matrix_recipe_yields_its_target(recipe):
    """every recipe of tests/kernel_matrix.py: the decision names its target; a recipe behind an environment switch hands the switch over"""
    text, plan = decide_recipe(recipe)
    assert plan is not None and text == recipe["target"], (text, plan)
    assert plan["fusedBatches"] == int(recipe["fused"])


def decide_recipe(recipe, fused_batches=None):
    """(kernel name, plan) of a recipe of tests/kernel_matrix.py as make_gpu sets it up: the handle's own tables (9001 steps)"""
    d, tabs = K.DOMAINS[recipe["domain"]]()
    env = {k: int(v) for k, v in recipe["env"].items()} or None
    kind = "fused" if recipe["fused"] else "plain"
    s = S.setup(K.PARAMS[recipe["params"]], tabs[0].n_entries, S.DEFAULT_INV, kind, recipe["kernel"], recipe["place"])
    nb = int(recipe["fused"]) if fused_batches is None else fused_batches
    return B.plan_launch(S.facts(d, env), s, stream=kind, fused_batches=nb, env=env)


# ---- the LDS edges --------------------------------------------------------------------------------------------------------------------
# (flag of the plan, rows of the sweep, last size with the flag, first without): the pairs of the recorded launches
EDGE_PAIRS = [
    ("ldsTallies", "edge/ldsTallies/{}", 314, 315),
    ("ldsVolume", "edge/ldsVolume/{}", 261, 262),
    ("ldsIntensity", "edge/ldsIntensity/{}", 84, 85),
    ("ldsGrid", "edge/ldsGrid/{}", 450, 451),
    ("tableInLds", "edge/tableInLds/{}", 193, 194),          # (plain launches: the 16 KB of start stores beside the table)
    ("tableInLds", "edge/tableInLds fused/{}", 311, 312),    # (fused launches: no start stores)
    ("ldsTrackSums", "track/{}", 384, 385),
]


@pytest.mark.parametrize("flag,rows,on,off", EDGE_PAIRS, ids=[e[1].split("/{}")[0] for e in EDGE_PAIRS])
def test_lds_edge_is_the_recorded_pair_of_sizes(flag, rows, on, off):
    """each LDS region at the last size that has it and the first that does not: an exact pair, in the golden and from the decision"""
    assert off == on + 1
    at = B.PLAN_NAMES.index(flag)
    by_id = {r["id"]: r for r in S.ROWS}
    for k, want in ((on, 1), (off, 0)):
        assert GOLDEN["rows"][rows.format(k)]["plan"][at] == want, (flag, k)
        assert S.decide(by_id[rows.format(k)])[1][flag] == want, (flag, k)
    # ... and nothing recorded contradicts it: on up to the pair, off from it (while the field stays where it is)
    for rid, rec in GOLDEN["rows"].items():
        head, _, k = rid.rpartition("/")
        if head + "/{}" == rows and "plan" in rec and rec["plan"][B.PLAN_NAMES.index("place")] == GOLDEN["rows"][rows.format(on)]["plan"][B.PLAN_NAMES.index("place")]:
            assert rec["plan"][at] == int(int(k) <= on), rid


# ---- the running estimate is an upper bound of what a launch allocates ------------------------------------------------------------
def _clear_geometry(nx, ny):
    s = 0
    while (((nx - 1) >> s) + 1) * (((ny - 1) >> s) + 1) > 1024:
        s += 1
    return s, ((nx - 1) >> s) + 1


def _plan_end_bytes(facts, nd, plan, replay=False):
    """lds_plan's end (i3rc_hip_lds_plan_words) for the decision's flags at four waves, without start stores and table"""
    direct = int(nd > 0 and plan["rayQueueCap"] == 0)
    queues = int(nd > 0 and not replay)          # (the replay build keeps the nested local estimate: no queues)
    q = np.array([facts["nx"], facts["ny"], facts["nz"], facts["ncomp"], nd, plan["ldsTallies"], plan["ldsIntensity"], plan["rayQueueCap"],
                  facts["clearNx"], facts["clearShift"], queues, direct, plan["place"], int(nd > 0), 4, 0, plan["ldsVolume"], 0], np.int32)
    out = np.zeros(13, np.int32)
    assert B.load().i3rc_hip_lds_plan_words(q.ctypes.data_as(B.ip), len(q), out.ctypes.data_as(B.ip), len(out)) == 0
    return 4 * int(out[10])


def _random_problem(rng):
    nx, ny, nz = (int(v) for v in rng.choice([1, 2, 3, 5, 8, 13, 31, 64, 100, 257, 700], 3))
    if rng.random() < 0.5:
        nx, ny, nz = (int(v) for v in rng.integers(1, 701, 3))
    ncomp, nd = int(rng.integers(1, 4)), int(rng.integers(0, 9))
    shift, cnx = _clear_geometry(nx, ny)
    col = int(rng.random() < 0.4)
    facts = dict.fromkeys(B.FACT_NAMES, 0)
    facts.update(nx=nx, ny=ny, nz=nz, ncomp=ncomp, xyRegular=int(rng.random() < 0.7), zRegular=1, absorbing=int(rng.random() < 0.5),
                 uniformSsa=int(ncomp == 1), uniformPf=int(ncomp == 1), columnRecords=col, columnBase=int(col and rng.random() < 0.5),
                 clearShift=shift, clearNx=cnx, clearWords=cnx * (((ny - 1) >> shift) + 1), maxPfIndex=1)
    place = str(rng.choice(["auto", "auto", "linear", "bricks"] + (["columns"] if col else [])))
    kernel = str(rng.choice(["auto", "general", "lane", "ring"]))
    params = dict(intensityMus=[0.5] * nd) if nd else {}
    return facts, nd, S.setup(params, 1, S.SMALL_INV, "plain", kernel, place, bool(rng.random() < 0.8))


def test_estimate_is_never_below_the_carve_up():
    """The estimate the decisions are made with (launch_plan.hpp, LdsEstimate) against lds_plan's end for the same flags at four waves,
    without start stores and table -- the "upper bound" its comment claims -- over the sweep and 400 seeded random shapes (sizes
    1 - 700, 0 - 8 directions, 1 - 3 components)."""
    checked = 0
    for row in S.ROWS:
        d, _ = S.domain(row["domain"])
        text, plan = S.decide(row)
        if plan is not None:
            facts = S.facts(d)
            assert plan["ldsEstimate"] >= _plan_end_bytes(facts, S.directions(row["params"]), plan, row["kind"] == "replay"), (row["id"], plan)
            checked += 1
    assert checked >= 200
    rng = np.random.default_rng(20261019)
    ran = 0
    for _ in range(400):
        facts, nd, s = _random_problem(rng)
        text, plan = B.plan_launch(facts, s)
        if plan is None:
            assert "LDS" in text, text
            continue
        ran += 1
        assert plan["ldsEstimate"] >= _plan_end_bytes(facts, nd, plan), (facts, s, plan)
    assert ran >= 150, ran


# ---- the facts of a field ---------------------------------------------------------------------------------------------------------------
def _cloud():
    from tools import cases

    return cases.step_cloud(ssa=1.0, nlayers=8, ncolumns=16)


def _gas(c, empty_ssa):
    gas = np.full_like(c["ext"], f32(2e-3))
    gas[:, :, ::3] = 0.0
    gas[3] = 0.0
    return gas, np.where(gas > 0, f32(1.0), f32(empty_ssa)).astype(f32), np.where(gas > 0, 1, 0).astype(np.int32)


def test_absorbing_follows_the_components_a_cell_can_select():
    """the cases the rule's comment names: a gas with omega = 0 in its empty cells does not make a conservative domain absorbing as the
    first component and does as the last; a conservative domain is not absorbing; an absorbing cloud is"""
    c = _cloud()
    gas, ssa, pf = _gas(c, 0.0)
    assert S.facts(dict(c, ext=[gas, c["ext"]], ssa=[ssa, c["ssa"]], pf=[pf, c["pf"]]))["absorbing"] == 0
    assert S.facts(dict(c, ext=[c["ext"], gas], ssa=[c["ssa"], ssa], pf=[c["pf"], pf]))["absorbing"] == 1
    gas, ssa, pf = _gas(c, 1.0)
    assert S.facts(dict(c, ext=[c["ext"], gas], ssa=[c["ssa"], ssa], pf=[c["pf"], pf]))["absorbing"] == 0
    assert S.facts(c)["absorbing"] == 0
    assert S.facts(dict(c, ssa=np.where(c["ext"] > 0, f32(0.99), f32(1.0)).astype(f32)))["absorbing"] == 1
    # (omega < 1 only where there is no extinction: never read)
    assert S.facts(dict(c, ssa=np.where(c["ext"] > 0, f32(1.0), f32(0.0)).astype(f32)))["absorbing"] == 0


def test_uniform_albedo_and_entry_are_taken_over_cells_with_extinction():
    c = _cloud()
    c = dict(c, ext=np.where(np.arange(c["ext"].shape[0])[:, None, None] < 2, f32(0.0), c["ext"]).astype(f32))
    clear = c["ext"] == 0
    assert clear.any() and not clear.all()
    f = S.facts(dict(c, ssa=np.where(clear, f32(0.0), f32(0.97)).astype(f32), pf=np.where(clear, 0, 1).astype(np.int32)))
    assert (f["uniformSsa"], f["uniformPf"], f["cellRecordBytes"]) == (1, 1, 0)
    pf = np.where(clear, 0, 1).astype(np.int32)
    pf[~clear & (np.arange(pf.shape[2]) % 2 == 0)[None, None, :]] = 2
    f = S.facts(dict(c, pf=pf))
    assert (f["uniformSsa"], f["uniformPf"], f["cellRecordBytes"]) == (1, 0, 0)
    ssa = np.where(np.arange(pf.shape[2]) % 3 == 0, f32(0.9), f32(0.99))[None, None, :] * np.ones_like(c["ssa"])
    f = S.facts(dict(c, ssa=ssa.astype(f32)))
    assert (f["uniformSsa"], f["uniformPf"], f["cellRecordBytes"]) == (0, 1, 0)
    # neither shared: the 8-byte records, unless the process has them switched off
    f = S.facts(dict(c, ssa=ssa.astype(f32), pf=pf))
    assert (f["uniformSsa"], f["uniformPf"], f["cellRecordBytes"]) == (0, 0, 8)
    assert S.facts(dict(c, ssa=ssa.astype(f32), pf=pf), env={"I3RC_CELL_RECORDS": 0})["cellRecordBytes"] == 0


@pytest.mark.parametrize("ncomp,want", [(1, 0), (2, 16), (3, 32), (4, 0)])
def test_cell_record_bytes(ncomp, want):
    """one decision: shared values (no records) for one component, 16 / 32 bytes for two / three, none beyond; an entry >= 65536 in
    one of the two components that share a word: none"""
    c = _cloud()
    def dom(entry, at=0):
        pfs = [np.ones(c["ext"].shape, np.int32) for _ in range(ncomp)]
        pfs[at] = np.full(c["ext"].shape, entry, np.int32)
        return dict(c, ext=[c["ext"]] * ncomp, ssa=[c["ssa"]] * ncomp, pf=pfs) if ncomp > 1 else dict(c, pf=pfs[0])
    assert S.facts(dom(1))["cellRecordBytes"] == want
    if ncomp in (2, 3):
        for at in (0, 1):
            assert S.facts(dom(65535, at))["cellRecordBytes"] == want
            f = S.facts(dom(65536, at))
            assert f["cellRecordBytes"] == 0 and f["maxPfIndex"] == 65536
        assert S.facts(dom(1), env={"I3RC_CELL_RECORDS": 0})["cellRecordBytes"] == 0
    if ncomp == 3:
        assert S.facts(dom(65536, 2))["cellRecordBytes"] == 32   # (the third entry has a word of its own)


def test_regular_spacing_flags_at_the_tolerance():
    """x / y: within 2 spacing(edge) of the first width; z: within 1 spacing"""
    c = _cloud()
    def moved(key, steps):
        e = c[key].astype(f32).copy()
        i = len(e) - 1
        for _ in range(abs(steps)):
            e[i] = np.nextafter(e[i], f32(np.inf if steps > 0 else -np.inf))
        return dict(c, **{key: e})
    base = S.facts(c)
    assert (base["xyRegular"], base["zRegular"]) == (1, 1)
    def flags(d):
        f = S.facts(d)
        return f["xyRegular"], f["zRegular"]
    # the last edge moved by float32 steps: spacing(edge) is one such step (the edge is no power of two)
    xe = float(c["xe"][-1])
    assert np.log2(xe) % 1 != 0 and np.log2(float(c["ze"][-1])) % 1 != 0
    assert flags(moved("xe", 2)) == (1, 1) and flags(moved("xe", -2)) == (1, 1)
    assert flags(moved("xe", 3)) == (0, 1) and flags(moved("xe", -3)) == (0, 1)
    if len(c["ye"]) > 2:
        assert flags(moved("ye", 2)) == (1, 1) and flags(moved("ye", 3)) == (0, 1)
    assert flags(moved("ze", 1)) == (1, 1) and flags(moved("ze", -1)) == (1, 1)
    assert flags(moved("ze", 2)) == (1, 0) and flags(moved("ze", -2)) == (1, 0)


def test_an_unknown_switch_is_refused():
    with pytest.raises(KeyError):
        S.facts(_cloud(), env={"I3RC_NO_SUCH_SWITCH": 1})
