"""Every production instantiation of photon_kernel traces the general kernel's photons (tests/kernel_matrix.py: one recipe each).

For each recipe the target must be the kernel that ran -- i3rc_hip_last_kernel_name, set from the dispatch-table entry that was
launched, equals the recipe's name exactly -- and it must give what the plainest launch gives on the same seeds: the general kernel,
the field read linearly, every tally straight to global memory (fused targets: one such launch per batch).  "The same photons, the
same fate": identical work counters and tallies equal to the order of their float64 additions (tests/sums.py), at photon counts
where a launch's chunks and workgroups end unevenly.  One-direction targets are also tied to the ring kernels.  The general kernel
itself is tied to the CPU oracle once per domain and problem kind of the table (test_general_kernel_on_the_matrix_domains_against_the_oracle)."""
import json
import os
import subprocess
import sys

import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.sums import assert_same_sums
from tests.test_launch_plan_cpu import decide_recipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (17, 5)
N_BIG = 30_001          # a multiple of neither the 256-photon chunk nor the 1024-thread workgroup
PLAIN_COUNTS = (1, 257, N_BIG)
FUSED_LOOPS = ((3, N_BIG), (1, 257), (1, 1))   # (batches, photons per batch)


def _integrator(recipe):
    from tests.test_gpu_parity import make_gpu

    d, tabs = K.DOMAINS[recipe["domain"]]()
    return make_gpu(d, tabs, **K.PARAMS[recipe["params"]])


def _plain(g, n, k=0):
    return g.computeRadiativeTransfer(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*K.SOURCE, n))


def _same(a, b, n, nd, what):
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    assert a["counters"]["photons"] == n, (what, a["counters"])
    assert_same_sums(a["raw"], b["raw"], a["counters"], directions=nd, what=what)


def check_recipe(recipe):
    """run one recipe's target and its references on the device; raises AssertionError on any difference"""
    target, nd = recipe["target"], K.directions(recipe["params"])
    g = _integrator(recipe)
    g.set_tuning(kernel=recipe["kernel"])
    g.select_grid_place(recipe["place"])
    loops = FUSED_LOOPS if recipe["fused"] else tuple((1, n) for n in PLAIN_COUNTS)
    got = {}
    for nb, n in loops:
        if recipe["fused"]:
            g.set_batch_fusion(1)
            got[nb, n] = g.computeRadiativeTransferBatches(SEED, nb, *K.SOURCE, n)
        else:
            got[nb, n] = [_plain(g, n)]
        assert g.kernel_name() == target, (target, g.kernel_name(), nb, n)
        # ... and the host-only decision entry, fed the same facts and knobs, reports the plan and the name this launch recorded
        # (the chunk needs the device: left out)
        name, plan = decide_recipe(recipe, fused_batches=nb if recipe["fused"] else 0)
        launched = g.last_plan()
        assert name == g.kernel_name() and {k: plan[k] for k in launched if k != "chunk"} == {k: v for k, v in launched.items() if k != "chunk"}, (target, name, plan, launched)
    assert all(v[0]["counters"]["scatterings"] > 0 for (nb, n), v in got.items() if n == N_BIG), target
    # the reference: general kernel, linear field, tallies straight to global memory, one plain launch per batch
    g.set_batch_fusion(0)
    g.set_tuning(kernel="general")
    g.select_grid_place("linear")
    g.set_lds_tallies(False)
    want = f"photon_kernel<PhiloxStream, {'true' if nd else 'false'}, true, GRID_GLOBAL{', one direction' if nd == 1 else ''}>"
    variants = [("general", want)]
    if nd == 1:   # ... and the event ring on the same photons
        variants.append(("ring", None))
    for kernel, name in variants:
        g.set_tuning(kernel=kernel)
        for (nb, n), runs in got.items():
            for k in range(nb):
                ref = _plain(g, n, k)
                if name:
                    assert g.kernel_name() == name, (target, g.kernel_name())
                else:
                    assert "one direction" not in g.kernel_name() and "GRID_GLOBAL" in g.kernel_name(), (target, g.kernel_name())
                _same(runs[k], ref, n, nd, (target, kernel, nb, n, k))
    g.finalize_Integrator()


IN_PROCESS = [r for r in K.RECIPES if not r["env"]]
ENVS = sorted({json.dumps(r["env"], sort_keys=True) for r in K.RECIPES if r["env"]})


@pytest.mark.parametrize("recipe", IN_PROCESS, ids=[r["target"].replace("photon_kernel", "") for r in IN_PROCESS])
def test_instantiation_traces_the_general_kernels_photons(recipe):
    check_recipe(recipe)


_CHILD = """
import json, sys
sys.path.insert(0, %r)
import torch  # noqa: F401  (the runtime order of tests/conftest.py)
from tests import kernel_matrix as K
from tests.test_gpu_kernel_matrix import check_recipe
env = json.loads(sys.argv[1])
done = []
for r in K.RECIPES:
    if r["env"] == env:
        check_recipe(r)
        done.append(r["target"])
print(json.dumps(done))
"""


def test_instantiations_behind_environment_switches():
    """Targets that only a variable read once per process reaches run in children of their own, one per environment, one after
    another; a child that ends abnormally ends the test before anything else starts on the device."""
    assert 1 <= len(ENVS) <= 4, ENVS
    for env in ENVS:
        e = json.loads(env)
        child_env = dict(os.environ, **e)
        try:
            p = subprocess.run([sys.executable, "-c", _CHILD % ROOT, env], env=child_env, capture_output=True, text=True, timeout=200)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{e}: the child ran beyond 200 s")
        if p.returncode != 0:
            pytest.fail(f"{e}: child exited with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        done = json.loads(p.stdout.strip().splitlines()[-1])
        assert sorted(done) == sorted(r["target"] for r in K.RECIPES if r["env"] == e), (e, done)


# ---- the general kernel against the oracle, once per (domain, flux / radiance) of the table ---------------------------------------
ANCHORS = sorted({(r["domain"], K.directions(r["params"]) > 0) for r in K.RECIPES})


@pytest.mark.parametrize("domain,radiance", ANCHORS, ids=[f"{d}-{'radiance' if rad else 'flux'}" for d, rad in ANCHORS])
def test_general_kernel_on_the_matrix_domains_against_the_oracle(oracle, domain, radiance):
    """Two-stage 3-sigma parity (tests/test_gpu_parity._parity; a first miss is recorded) of the general kernel -- which every recipe
    is tied to -- with the CPU oracle on the same tables: flux with absorption and a surface; radiance with roulette, hybrid tables
    and the contribution limit."""
    from tests.test_gpu_features import _intensity_pair
    from tests.test_gpu_parity import _parity, make_gpu, make_oracle

    d, tabs = K.DOMAINS[domain]()
    n_table = 9001
    if radiance:
        p = K.PARAMS["ring hybrid"]
        gp = {k: v for k, v in p.items() if k not in ("intensityMus", "intensityPhis", "hybridPhaseFunWidth")}
        op = dict(surfaceAlbedo=p["surfaceAlbedo"], useRRForIntensity=1, zetaMin=p["zetaMin"], useHybrid=1,
                  numOrdersOrig=p["numOrdersOrigPhaseFunIntenCalcs"], limitContrib=1, maxContrib=p["maxIntensityContribution"])
        g, o = _intensity_pair(oracle, d, tabs, n_table=n_table, gpu_params=gp, oracle_params=op, mus=p["intensityMus"],
                               phis=p["intensityPhis"], hybrid_width=p["hybridPhaseFunWidth"])
        keys = ("intensity", "fluxUp")
    else:
        inv = [t.inverse_table(n_table) for t in tabs]
        g = make_gpu(d, tabs, **K.PARAMS["flux"])
        for c, t in enumerate(inv):
            g.set_tables(c + 1, inverse=t)
        o = make_oracle(oracle, d, inv)
        o.specify(**K.PARAMS["flux"])
        keys = ("fluxUp", "fluxDown", "fluxAbsorbed")
    g.set_tuning(kernel="general")
    # (batches of 2e4 photons: the column clouds' narrowest columns see a few hundred each, and their batch means are near normal)
    n = 20_000
    gr, _ = _parity(oracle, g, o, 10, n, K.SOURCE[0], az=K.SOURCE[1], keys=keys, floor=1e-6)
    assert ", true, GRID_" in g.kernel_name(), g.kernel_name()
    assert all(r["counters"]["photons"] == n for r in gr)
    assert sum(float(r["volumeAbsorption"].sum()) for r in gr) > 0   # (absorption was tallied)
    g.finalize_Integrator()
