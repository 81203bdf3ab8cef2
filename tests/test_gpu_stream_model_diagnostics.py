"""The four diagnostic tallies -- level fluxes, actinic flux by track length, path-length moments, the path histogram -- against the
float64 stream model (tests/stream_model.py, Problem.extra): the same seed and photon numbers on both sides, every counter equal, every
entry of the kind's block within the model's own propagated float32 bound, entry by entry.

What this pins that no other test does: a single entry of a diagnostic block once a photon has scattered -- pathUp2 of one column, the
track length of one cell with the weight BEFORE the event at the piece's end, the column in which a scattered segment crosses level k,
the bin a multiply scattered photon's float(L) falls in.  The suites of the kinds themselves hold identities between two tallies of the
same kernel (both sides share pathLen, the LENGTH pieces, w and the column), closed forms for unscattered light and domain means within
4 standard errors; this module holds the five photon_kernel<Philox{Level,Track,Path,Bin}Stream, false, true, GRID> instantiations and the
LENGTH tracer variants only they compile to an independent answer.

A path has no upper limit, so nothing caps what a fragile photon might carry into a path sum, a bin or a cell: the blocks are compared
over the photons that are NOT fragile, the kind's own decisions (start column, level column, bin) among the reasons.  Per case and kind
every maximal run of at least 64 such photons is launched with its own firstPhoton into one accumulated block, then fetched once; the
model run over exactly those photons is the expected value, with no allowance for the counters and the float32 bound alone for every
tally.  The cases are the shared flux cases at their own sizes (20 000 photons, 4 x 3 columns, 8 layers); S.DIAGNOSTIC_WIDE says which
run under columns a hundred times as wide for which kind, S.BIN_EDGES the histogram's edges, S.DIAGNOSTIC_FIRST the one case that runs
other photons than 0 .. 19 999 (the conditions that decide it are asserted in tests/test_stream_model_cpu.py).

Measured on an MI355X (the module: 35 tests in 5 s): every counter of every run equal to the model's, and the largest difference as a
fraction of the propagated float32 bound ALONE, per case and kind (runs launched, photons in them | the kind's fields | fragile share with
the kind's own decisions, S.DIAGNOSTIC_SHARES; the old tallies of the same launches: 0.01 ... 0.36, as in tests/test_gpu_stream_model.py):
                 levels: Up, Down              tracks: cells, layer sums     paths: Up1, Up2, Down1, Down2             bins: Up, PathUp, Down, PathDown
  a absorbing    57, 19650 | 0.063 0.10  | .0035   26, 19967 | 0.011 0.0032 | .0013   26, 19967 | .0006 .0008 .0014 .0028 | .0013   49, 19542 | 0.17 .0094 0.15 .0079 | .0031
  b records      47, 19625 | 0.042 0.19  | .0028   12, 19989 | 0.18  0.010  | .00055  26, 19909 | .0008 .0027 .0013 .0026 | .00135  60, 19416 | 0.13 .0057 0.13 .0086 | .00385
  c two          63, 19156 | 0.16  0.13  | .0045   39, 19608 | 0.0026 0.0008 | .00245 39, 19608 | .0010 .0010 .0004 .0006 | .00245  67, 19282 | 0.33 .0019 0.28 .0035 | .00445
  e irregular    25, 19916 | 0.098 0.019 | .00125  38, 19822 | 0.0063 0.0018 | .00225 38, 19822 | .0008 .0011 .0010 .0021 | .00225  47, 19391 | 0.074 .0077 0.090 .0070 | .0031
  f no roulette  38, 19882 | 0.039 0.089 | .0020   68, 19239 | 0.026 0.012  | .00455  68, 19239 | .0027 .0113 .0034 .0071 | .00455  67, 19420 | 0.17 .0079 0.12 .0134 | .0042
  g black        38, 19821 | 0.036 0.016 | .0022   17, 19984 | 0.0091 0.0042 | .0008  17, 19984 | .0009 .0010 .0034 .0062 | .0008   56, 19667 | 0.10 .0069 0.085 .0527 | .00315
  g white        36, 19603 | 0.016 0.024 | .00215  17, 19903 | 0.052 0.0022 | .00095  72, 19246 | .0005 .0007 .0004 .0009 | .00435  55, 19104 | 0.087 .0113 0.084 .0054 | .0038
  a common, bins (65 runs, 19023 photons): binUp and binDown equal to the bit, binPathUp 0.0092, binPathDown 0.0063 | .0046
  a absorbing, sums in LDS | on global atomics: tracks 0.011, 0.0032 both ways; bins 0.17 .0094 0.15 .0079 both ways
  a absorbing, photons from 2^32 - 700 (7, 4, 4, 6 runs; 1411 ... 1497 photons): levels 0.089 0.11; tracks 0.025 0.0029; paths .0013 .0015 .0043 .0042;
  bins 0.23 .016 0.23 .016
(the path sums sit at a thousandth of their bound: it carries the model's along-path error e_s of every segment, which is generous for
a quantity that does not depend on where a segment ends sideways).  No difference beyond a bound: no finding in a kernel or a comment."""
import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import stream_model as S
from tests.test_gpu_stream_model import _integrator
from tests.test_stream_model_cpu import diagnostic_clean, diagnostic_runs

pytestmark = pytest.mark.gpu

LEAST = 64                  # the shortest run of photons launched on its own
TAG = {"levels": "PhiloxLevelStream", "tracks": "PhiloxTrackStream", "paths": "PhiloxPathStream", "bins": "PhiloxBinStream"}
OLD = ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption")


def _switch(name, kind):
    """the one specifyParameters switch of the kind"""
    return {"levels": dict(computeLevelFluxes=True), "tracks": dict(computeActinicFlux=True), "paths": dict(computePathLengths=True),
            "bins": dict(pathHistogramEdges=S.bin_edges(name))}[kind]


def _diagnostic_integrator(monkeypatch, name, kind):
    """test_gpu_stream_model._integrator on the case as the kind runs it (S.diagnostic_case: its own columns or wide ones), registered
    under a name of its own for the length of the test, with the kind switched on"""
    key = f"{name} [{kind}]"
    monkeypatch.setitem(S.CASES, key, S.diagnostic_case(name, kind))
    g = _integrator(key)
    g.specifyParameters(**_switch(name, kind))
    return g


def _launch_runs(g, runs):
    """every run with its own firstPhoton into one accumulated block, one finish()"""
    zero = True
    for first, count in runs:
        g.launch(M.new_RandomNumberSequence(S.SEED), M.new_PhotonStream(*S.SUN, count), firstPhoton=first, zero=zero)
        zero = False
    return g.finish()


def _shaped(g, res, model, kind):
    """a run's raw tallies in the model's shapes: the old fields by the layout, the kind's block behind the counters field after field
    (tally_block.hpp: tally_layout, path_bin_field), and the track sums added over the columns of every layer"""
    lay, raw = g.layout(), res["raw"]
    out = {k: raw[getattr(lay, k):getattr(lay, k) + model.tallies[k].size].reshape(model.tallies[k].shape) for k in OLD}
    at = lay.counters + M.binding.NUM_COUNTERS
    for k in S.EXTRA_FIELDS[kind]:
        out[k] = raw[at:at + model.tallies[k].size].reshape(model.tallies[k].shape)
        at += model.tallies[k].size
    assert at == lay.total == len(raw), (at, lay.total, len(raw))
    if kind == "tracks":
        out["trackLayers"] = out["tracks"].sum(axis=(1, 2))
    return out


def _hold(g, res, model, kind, what):
    """every counter equal, every tally -- the old ones, the kind's block entry by entry, the per-layer track sums -- within the float32
    bound alone; prints the largest difference / bound per field"""
    assert not model.per_photon["fragile"].any()
    got = _shaped(g, res, model, kind)
    assert set(got) == set(model.tallies), (set(got), set(model.tallies))
    miss, worst = S.compare(model, got, res["counters"])
    print(f"{what}: kernel {g.kernel_name()} photons {model.n} largest difference / float32 bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert miss == [], (what, g.kernel_name(), miss)
    assert TAG[kind] in g.kernel_name() and ", true, GRID_" in g.kernel_name(), g.kernel_name()
    return got


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("name", S.DIAGNOSTIC_CASES)
def test_diagnostic_block_against_the_model(name, kind, monkeypatch):
    runs = diagnostic_runs(name, kind, least=LEAST)
    model = diagnostic_clean(name, kind, least=LEAST)
    assert model.n == sum(c for _, c in runs) >= 0.9 * S.CASES[name]["n"], (model.n, len(runs))
    g = _diagnostic_integrator(monkeypatch, name, kind)
    got = _hold(g, _launch_runs(g, runs), model, kind, f"{name} [{kind}] {len(runs)} runs")
    assert all(np.count_nonzero(got[k]) > 0 for k in S.EXTRA_FIELDS[kind] if model.tallies[k].any())
    g.finalize_Integrator()


def test_bins_of_whole_weights_are_equal_exactly(monkeypatch):
    """a conservative medium: every weight a tally sees is 1 or float32(albedo) -- sums of those are exact in float64 in any order,
    so the weight bins are the model's to the bit"""
    name, kind = "a common", "bins"
    runs, model = diagnostic_runs(name, kind, least=LEAST), diagnostic_clean(name, kind, least=LEAST)
    g = _diagnostic_integrator(monkeypatch, name, kind)
    got = _hold(g, _launch_runs(g, runs), model, kind, f"{name} [{kind}] {len(runs)} runs")
    for k in ("binUp", "binDown"):
        assert np.array_equal(got[k], model.tallies[k]), (k, np.flatnonzero(got[k] != model.tallies[k]))
    g.finalize_Integrator()


@pytest.mark.parametrize("kind", ["tracks", "bins"])
def test_sums_in_lds_and_on_global_atomics(kind, monkeypatch):
    """`a absorbing` once with the workgroup's sums in LDS and once with every sum straight to global memory (set_lds_tallies, the
    switch of the kinds' own suites); the plan says which"""
    name = "a absorbing"
    word = "ldsTrackSums" if kind == "tracks" else M.binding.PLAN_BIN_NAME
    runs, model = diagnostic_runs(name, kind, least=LEAST), diagnostic_clean(name, kind, least=LEAST)
    g = _diagnostic_integrator(monkeypatch, name, kind)
    for lds in (True, False):
        g.set_lds_tallies(lds)
        res = _launch_runs(g, runs)
        assert g.last_plan()[word] == int(lds) and g.last_plan()["ldsTallies"] == int(lds), g.last_plan()
        _hold(g, res, model, kind, f"{name} [{kind}] sums {'in LDS' if lds else 'on global atomics'}")
    g.finalize_Integrator()


@pytest.mark.parametrize("kind", S.KINDS)
def test_photon_numbers_across_two_to_the_32(kind, monkeypatch):
    """photons from 2^32 - 700 on: the runs without a fragile photon below and beyond 2^32 -- pathLen and izFrom start afresh whatever
    the photon's high word is"""
    name, first, n = "a absorbing", 2 ** 32 - 700, 1500
    runs = diagnostic_runs(name, kind, first=first, n=n, least=LEAST)
    model = diagnostic_clean(name, kind, first=first, n=n, least=LEAST)
    below, beyond = sum(c for a, c in runs if a + c <= 2 ** 32), sum(a + c - max(a, 2 ** 32) for a, c in runs if a + c > 2 ** 32)
    assert below >= 300 and beyond >= 300, (runs, below, beyond)
    g = _diagnostic_integrator(monkeypatch, name, kind)
    _hold(g, _launch_runs(g, runs), model, kind, f"{name} [{kind}] photons from 2^32 - 700")
    g.finalize_Integrator()
