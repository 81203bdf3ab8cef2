"""The path-length histogram of reflected and transmitted light on the device: the block of 4 (nBins + 1) float64 words that
photon_kernel<PhiloxBinStream, false, true, GRID> fills -- per bin of the photon's geometric path L the sums of w and of w L over the
photons that fluxUp and fluxDown count, domain-wide, the last word of each field the overflow bin -- pinned by identities against
tallies the project already trusts, by exact sums and by an independent solver.

  same photons     feature on against the general kernel with it off and against path lengths on: every counter identical, the old
                   tallies equal to the order of their float64 additions (tests/sums.py), the bins' sums the flux and path sums, every
                   bin's mean path between its edges; once per place of the extinction field, and with a source inside the domain
  exact            no extinction, a black surface: every photon travels the same path L0 with weight 1 -- whole numbers and equal
                   terms, whose sums are exact in any order -- between two edges, on an edge, beyond the last edge, with 1 and with
                   1024 bins, the sums in LDS and in global memory bit for bit
  reflection       the same domain over albedo 1: the path goes on through the reflection
  LDS / global     the same block either way, and which one a launch did
  equivalence      R(k) / R(0) = <exp(-k L)> from one conservative run, bracketed bin by bin, against the adding-doubling solver with
                   the absorber in it
  launches         tiny and split batches, accumulation, zeroing; the refusals; the Fortran shell

Tolerances.  Two runs of the same photons: tests/sums.py.  Exact sums: 2^-52 per term of a float64 sum.  A bin's mean path: the bin's
edges, widened by 2^-24 (the rule bins float32(L)) and the sums' bound.  The solver comparison: 4 standard errors of the batch means
around a bracket whose half-width must stay below a quarter of a standard error."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K
from tests.extra_tally import N, old as _old, run
from tests.sums import assert_same_sums, order_rtol
from tests.test_gpu_parity import hg_table, make_gpu
from tests.test_gpu_path_lengths import SLAB_Z, _clear_domain, _straight_path
from tools import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = (31, 4)
_run = functools.partial(run, seed=SEED)
FIELDS = ("binUp", "binPathUp", "binDown", "binPathDown")
NAMES = M.host.PATH_HISTOGRAM_NAMES
BIN_WORD = M.binding.PLAN_BIN_NAME


def _geometric(first, ratio, nbins):
    """nBins + 1 float32 edges: 0, then a geometric progression from `first`"""
    e = np.concatenate([[0.0], first * np.float64(ratio) ** np.arange(nbins)]).astype(np.float32)
    assert e.size == nbins + 1 and (np.diff(e) > 0).all() and np.isfinite(e).all()
    return e


def _block(g, res):
    """the four raw fields, nBins + 1 words each, as views of a result's packed buffer, by name"""
    *offs, nbins, total = g.path_histogram_layout()
    first = g.layout().counters + M.binding.NUM_COUNTERS
    assert nbins == g.pathHistogramEdges.size - 1 and offs == [first + k * (nbins + 1) for k in range(4)], (offs, nbins)
    assert total == first + 4 * (nbins + 1) == len(res["raw"]) == g.layout().total, (total, len(res["raw"]))
    return {name: res["raw"][at:at + nbins + 1] for name, at in zip(FIELDS, offs)}


def _flux(g, res, which):
    at = getattr(g.layout(), which)
    return res["raw"][at:at + g.ny * g.nx]


def _one(x):
    return np.array([float(np.sum(x))])


def _check_bins(g, res, edges, counters):
    """what every block must satisfy: the bins add up to the fluxes, the overflow bin of these edges is empty, every bin's mean path
    lies between its edges, and the normalised arrays are the raw ones per photon"""
    blk = _block(g, res)
    assert_same_sums(_one(blk["binUp"]), _one(_flux(g, res, "fluxUp")), counters, what="the bins of fluxUp")
    assert_same_sums(_one(blk["binDown"]), _one(_flux(g, res, "fluxDown")), counters, what="the bins of fluxDown")
    assert all(blk[k][-1] == 0 for k in FIELDS), [blk[k][-1] for k in FIELDS]
    slack = 2.0 ** -24 + order_rtol(counters)
    e = edges.astype(np.float64)
    for w, wl in (("binUp", "binPathUp"), ("binDown", "binPathDown")):
        n, s = blk[w][:-1], blk[wl][:-1]
        assert (n >= 0).all() and ((n == 0) == (s == 0)).all() and np.count_nonzero(n) > 2, (w, n)      # (the light spreads over several bins)
        assert (e[:-1] * n * (1 - slack) <= s).all() and (s <= e[1:] * n * (1 + slack)).all(), (w, np.flatnonzero(~((e[:-1] * n * (1 - slack) <= s) & (s <= e[1:] * n * (1 + slack)))))
    for name, field in zip(NAMES, FIELDS):
        assert res[name].dtype == np.float32 and np.array_equal(res[name], np.float32(blk[field] / counters["photons"])), name
    return blk


# ---- 1: the same photons, once per place of the extinction field -------------------------------------------------------------------
CLOUD = dict(ssa=0.97, nlayers=16, ncolumns=32)
CLOUD_N = 200_000
CLOUD_EDGES = _geometric(2.5, 1.4, 80)          # from a hundredth of the cloud's 250 m to 1e12 m: no path is longer


def _same_photons(g, place, n, edges):
    g.set_tuning(kernel="general")
    off = _run(g, n=n)
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>", g.kernel_name()
    old_total = g.layout().total
    assert g.path_histogram_layout() == (-1, -1, -1, -1, 0, old_total) and BIN_WORD not in g.last_plan()
    g.specifyParameters(pathHistogramEdges=edges)
    on = _run(g, n=n)
    assert g.kernel_name() == f"photon_kernel<PhiloxBinStream, false, true, {place}>", g.kernel_name()
    plan = g.last_plan()
    assert plan[BIN_WORD] == 1 and plan["ldsTrackSums"] == 0 and plan["startStoreBytes"] == 0 and plan["tableInLds"] == 0, plan
    c = on["counters"]
    assert c == off["counters"] and c["photons"] == n and c["scatterings"] > 0 and c["surfaceHits"] > 0 and c["exitsTop"] > 0, (c, off["counters"])
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], c, what=("old tallies", place))
    assert g.layout().total == old_total + 4 * edges.size
    blk = _check_bins(g, on, edges, c)
    # path lengths on instead, same handle: the same photons, and the bins of w L add up to the columns' sums of w L
    g.specifyParameters(pathHistogramEdges=None)
    assert g.layout().total == old_total and g.path_histogram_layout() == (-1, -1, -1, -1, 0, old_total)
    g.specifyParameters(computePathLengths=True)
    paths = _run(g, n=n)
    assert "PhiloxPathStream" in g.kernel_name() and paths["counters"] == c
    up1, _, down1, _, _ = g.path_length_layout()
    ncol = g.nx * g.ny
    assert_same_sums(_one(blk["binPathUp"]), _one(paths["raw"][up1:up1 + ncol]), c, what=("the bins of pathUp1", place))
    assert_same_sums(_one(blk["binPathDown"]), _one(paths["raw"][down1:down1 + ncol]), c, what=("the bins of pathDown1", place))
    g.specifyParameters(computePathLengths=False)
    again = _run(g, n=n)                                                 # ... and off again: the old buffer, the old kernel
    assert g.kernel_name() == f"photon_kernel<PhiloxStream, false, true, {place}>" and again["counters"] == c and "pathHistogramUp" not in again
    assert_same_sums(again["raw"], off["raw"], c, what=("off again", place))
    g.finalize_Integrator()


@pytest.mark.parametrize("place", K.PLACES[:4])
def test_same_photons_on_the_step_cloud(place):
    g = make_gpu(cases.step_cloud(**CLOUD), hg_table(), surfaceAlbedo=0.3)
    g.select_grid_place(K.PLACE_KNOB[place])
    _same_photons(g, place, CLOUD_N, CLOUD_EDGES)


def test_same_photons_over_a_base_profile():
    """the fifth place -- column records over a base profile -- is read on domains of several components"""
    d, tabs = K.DOMAINS["colbase2"]()
    g = make_gpu(d, tabs, **K.PARAMS["flux"])
    g.select_grid_place(K.PLACE_KNOB["GRID_COLBASE"])
    depth = float(d["ze"][-1] - d["ze"][0])
    _same_photons(g, "GRID_COLBASE", N, _geometric(0.01 * depth, 1.4, 80))


def test_same_photons_with_a_source_inside_the_domain():
    """an explicit stream that starts photons at any height, half of them upwards"""
    g = make_gpu(cases.step_cloud(**CLOUD), hg_table(), surfaceAlbedo=0.3)
    rng = np.random.default_rng(5)
    n = 5_003
    mu = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.2, 1.0, n)
    arrays = [rng.random(n), rng.random(n), rng.uniform(0.02, 0.98, n), mu, rng.uniform(0, 2 * np.pi, n)]
    g.set_tuning(kernel="general")
    off = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    g.specifyParameters(pathHistogramEdges=CLOUD_EDGES)
    on = g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), M.PhotonStream(arrays=arrays))
    assert "PhiloxBinStream" in g.kernel_name()
    assert on["counters"] == off["counters"] and on["counters"]["photons"] == n
    assert_same_sums(_old(g, on), off["raw"][:len(_old(g, on))], on["counters"], what="explicit source")
    blk = _check_bins(g, on, CLOUD_EDGES, on["counters"])
    assert blk["binUp"][:8].sum() > 0                    # (photons that start upwards just below the top: paths far shorter than the cloud is deep)
    g.finalize_Integrator()


# ---- 2: exact ------------------------------------------------------------------------------------------------------------------------
EXACT_N = 100_003                                                       # no multiple of 64 or 256, several workgroups
L0 = _straight_path(SLAB_Z)                                             # the float64 path of every photon, just below 1
EXACT_EDGES = {
    "between two edges": np.array([0.0, 0.25, 0.5, 0.75, 0.9, 1.1, 2.0, 4.0, 8.0], np.float32),
    "on an edge": np.array([0.0, 0.5, f32(L0), 2.0], np.float32),       # edges[b] <= float32(L0): the bin whose lower edge it is
    "beyond the last edge": np.array([0.0, 0.25, 0.5], np.float32),
    "one bin": np.array([0.0, 2.0], np.float32),
    "1024 bins": np.linspace(0.0, 2.0, 1025).astype(np.float32),
}


def _exact_run(albedo, edges, n, lds):
    g = make_gpu(_clear_domain("1x1x4"), hg_table(), surfaceAlbedo=albedo, pathHistogramEdges=edges)
    g.set_lds_tallies(lds)
    res = _run(g, n=n, sun=(1.0, 0.0))
    assert g.last_plan()[BIN_WORD] == int(lds) and g.last_plan()["ldsTallies"] == int(lds) and "PhiloxBinStream" in g.kernel_name(), g.last_plan()
    blk = {k: v.copy() for k, v in _block(g, res).items()}
    g.finalize_Integrator()
    return res, blk


@pytest.mark.parametrize("case", list(EXACT_EDGES))
def test_straight_down_through_clear_air_is_exact(case):
    edges = EXACT_EDGES[case]
    nbins = edges.size - 1
    want = int(np.clip(np.searchsorted(edges, f32(L0), side="right") - 1, 0, nbins))
    assert want == {"between two edges": 4, "on an edge": 2, "beyond the last edge": nbins, "one bin": 0}.get(case, want) and (nbins < 1024 or 400 < want < 600)
    blocks = {}
    for lds in (True, False):
        res, blk = _exact_run(0.0, edges, EXACT_N, lds)
        c = res["counters"]
        assert c["photons"] == EXACT_N and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == EXACT_N and c["exitsTop"] == 0, c
        assert blk["binDown"][want] == EXACT_N
        # (each term is 1 x L0 formed in float64; the word is a sum of N equal terms: 2^-52 per term)
        err = abs(blk["binPathDown"][want] - EXACT_N * L0)
        print(case, "lds" if lds else "global", "bin", want, "error in units of 2^-52 per term", err / (EXACT_N * L0) * 2.0 ** 52 / EXACT_N)
        assert err <= EXACT_N * 2.0 ** -52 * (EXACT_N * L0), (err, L0)
        for k in FIELDS:
            rest = blk[k].copy()
            if k in ("binDown", "binPathDown"):
                rest[want] = 0.0
            assert (rest == 0).all(), (k, np.flatnonzero(rest))
        blocks[lds] = blk
    # sums of whole numbers and of equal terms are exact in any order: in LDS and in global memory the same bits
    for k in FIELDS:
        assert np.array_equal(blocks[True][k].view(np.uint64), blocks[False][k].view(np.uint64)), k


# ---- 3: through a reflection ---------------------------------------------------------------------------------------------------------
def test_the_path_goes_on_through_a_reflection():
    """The empty domain over albedo 1: every photon arrives at the surface once, with the path L0, is reflected with its weight 1 and
    leaves through the top after another leg that is longer than L0 (tests/test_gpu_path_lengths.py): float32(L) >= float32(2 L0)
    rounded down, which is an edge here, so every bin below that edge stays empty."""
    two = f32(2.0 * L0)
    two = two if float(two) <= 2.0 * L0 else np.nextafter(two, f32(0.0))
    edges = np.concatenate([[0.0, 0.5, 0.9, 1.1, 1.9], [two], float(two) * 1.5 ** np.arange(1, 60)]).astype(np.float32)
    assert (np.diff(edges) > 0).all()
    n = 20_003
    res, blk = _exact_run(1.0, edges, n, True)
    c = res["counters"]
    assert c["photons"] == n and c["dropped"] == 0 and c["scatterings"] == 0 and c["surfaceHits"] == n and c["exitsTop"] == n, c
    assert blk["binDown"][2] == n and abs(blk["binPathDown"][2] - n * L0) <= n * 2.0 ** -52 * (n * L0)      # unchanged: [0.9, 1.1)
    assert np.count_nonzero(blk["binDown"]) == 1 and np.count_nonzero(blk["binPathDown"]) == 1
    assert (blk["binUp"][:5] == 0).all() and (blk["binPathUp"][:5] == 0).all(), blk["binUp"][:8]
    assert blk["binUp"].sum() == n and blk["binUp"][5] > 0 and np.count_nonzero(blk["binUp"]) > 4      # (whole numbers: exact)
    assert blk["binPathUp"].sum() > 2 * L0 * n


# ---- 4: sums in LDS against global atomics -------------------------------------------------------------------------------------------
def test_lds_sums_against_global_atomics():
    g = make_gpu(cases.step_cloud(**CLOUD), hg_table(), surfaceAlbedo=0.3, pathHistogramEdges=CLOUD_EDGES)
    lds = _run(g, n=CLOUD_N)
    assert g.last_plan()[BIN_WORD] == 1 and g.last_plan()["ldsGrid"] == 1, g.last_plan()
    g.set_lds_tallies(False)
    glb = _run(g, n=CLOUD_N)
    assert g.last_plan()[BIN_WORD] == 0 and g.last_plan()["ldsTallies"] == 0 and "PhiloxBinStream" in g.kernel_name(), g.last_plan()
    assert glb["counters"] == lds["counters"]
    assert_same_sums(glb["raw"], lds["raw"], lds["counters"], what="sums in LDS against global atomics")
    _check_bins(g, glb, CLOUD_EDGES, glb["counters"])
    g.finalize_Integrator()


def test_no_room_in_lds_for_1024_bins():
    """A field of 32 KB in LDS leaves less than the 36.9 KB the sums and edges of 1024 bins take within a workgroup's budget: the launch
    adds to global memory.  64 bins over every sixteenth edge fit: their sums in LDS are the sums of sixteen of the others."""
    d = cases.step_cloud(ssa=0.97, nlayers=64, ncolumns=128)
    fine = _geometric(2.5, 1.03, 1024)
    coarse = fine[::16]
    n = 50_001
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3, pathHistogramEdges=fine)
    a = _run(g, n=n)
    plan = g.last_plan()
    assert plan[BIN_WORD] == 0 and plan["ldsGrid"] == 1 and plan["ldsTallies"] == 1 and g.kernel_name() == "photon_kernel<PhiloxBinStream, false, true, GRID_LDS>", plan
    blk_a = {k: v.copy() for k, v in _check_bins(g, a, fine, a["counters"]).items()}
    g.specifyParameters(pathHistogramEdges=coarse)
    b = _run(g, n=n)
    assert g.last_plan()[BIN_WORD] == 1 and g.last_plan()["ldsBytes"] > plan["ldsBytes"], g.last_plan()
    assert b["counters"] == a["counters"]
    blk_b = _check_bins(g, b, coarse, b["counters"])
    for k in FIELDS:
        assert_same_sums(blk_a[k][:-1].reshape(64, 16).sum(1), blk_b[k][:-1], a["counters"], what=("sixteen bins in one", k))
    g.finalize_Integrator()


# ---- 5: the equivalence theorem against the independent solver -------------------------------------------------------------------------
TAU_A = (0.05, 0.5, 2.0, 8.0)
H = 1.0
# a ratio of 1.01 from 0.01 H to 263 H, the 1024 bins the histogram takes: a bin's bracket is k^2 width^2 / 8 wide at most,
# 1.3e-5 (k L)^2 exp(-k L) of its share -- what the sharpest figure needs, the transmitted light under tau_a = 2 through tau_0 = 1, whose
# direct beam has one path, 2 H, and no scatter of its own (with a ratio of 1.0125 that half-width was 0.26 of a standard error)
THEOREM_EDGES = _geometric(0.01 * H, 1.01, 1024)


@functools.lru_cache(maxsize=None)
def _solver_ratios(tau, omega, albedo):
    """{tau_a: (fluxUp ratio, fluxDown ratio)}: the slab with a pure absorber of optical depth tau_a mixed in, over the slab without"""
    from tests.plane_parallel_solver import solve
    from tests.test_plane_parallel import G, MU0, _sampled_moments

    def F(t):
        r = solve(tau + t, omega * tau / (tau + t), G, MU0, albedo=albedo, chi=_sampled_moments())
        return np.array([r["fluxUp"], r["fluxDown"]])
    f0 = F(0.0)
    return {t: F(t) / f0 for t in TAU_A}


def _bracket(p, pl, edges, k):
    """(lower, upper) bound of <exp(-k L)> from a normalised histogram: p the bins' shares, pl those times the bins' mean paths"""
    p, pl, e = p.astype(np.float64), pl.astype(np.float64), edges.astype(np.float64)
    lo, hi = e[:-1], e[1:]
    has = p[:-1] > 0
    mean = np.clip(np.where(has, pl[:-1] / np.where(has, p[:-1], 1.0), lo), lo, hi)       # (the float32 rounding of the two arrays)
    lower = np.sum(p[:-1] * np.exp(-k * mean))                                           # convexity: Jensen, bin by bin
    chord = ((hi - mean) * np.exp(-k * lo) + (mean - lo) * np.exp(-k * hi)) / (hi - lo)
    upper = np.sum(p[:-1] * chord) + p[-1] * np.exp(-k * e[-1])                         # the overflow bin: between 0 and this
    total = p.sum()
    return lower / total, upper / total


@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("omega,albedo", [(0.9, 0.5), (1.0, 0.0)])
def test_equivalence_theorem_against_the_adding_solver(tau, omega, albedo):
    """Per (tau_a, direction): lower bound | upper bound | reference | standard error | half-width / standard error are printed.
    Left out: a pair whose reference ratio is below 1e-3 (the batch means of exp(-k L) are not Gaussian there) -- the transmitted
    light at tau_a = 8 at most."""
    from tests.test_plane_parallel import G, MOMENTS, MU0, SIGMAS

    nb, n = 20, 100_000
    ext = np.full((4, 1, 1), f32(tau / H), np.float32)
    d = dict(xe=np.array([0.0, 4.0], np.float32), ye=np.array([0.0, 4.0], np.float32), ze=SLAB_Z * f32(H), ext=ext,
             ssa=np.full_like(ext, f32(omega)), pf=np.ones(ext.shape, np.int32))
    g = make_gpu(d, hg_table(G, MOMENTS), surfaceAlbedo=albedo, minInverseTableSize=10001, pathHistogramEdges=THEOREM_EDGES)
    per = []
    for b in range(1, nb + 1):
        res = _run(g, n=n, seed=(12, b), sun=(MU0, 0.0))
        assert res["pathHistogramUp"][-1] < 1e-6 and res["pathHistogramDown"][-1] < 1e-6      # (next to nothing is longer than 263 H)
        per.append([_bracket(res[p], res[pl], THEOREM_EDGES, t / H) for t in TAU_A for p, pl in ((NAMES[0], NAMES[1]), (NAMES[2], NAMES[3]))])
    assert g.last_plan()[BIN_WORD] == 1
    g.finalize_Integrator()
    per = np.array(per).reshape(nb, len(TAU_A), 2, 2)                # batch, tau_a, direction, (lower, upper)
    mean, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(nb)
    want = _solver_ratios(tau, omega, albedo)
    left_out = []
    for i, t in enumerate(TAU_A):
        for j, name in enumerate(("fluxUp", "fluxDown")):
            ref = want[t][j]
            (lo, hi), (se_lo, se_hi) = mean[i, j], se[i, j]
            half = 0.5 * (hi - lo)
            print(f"tau {tau} omega {omega} albedo {albedo} tau_a {t} {name}: [{lo:.6e}, {hi:.6e}] reference {ref:.6e}, s.e. {se_lo:.2e} / {se_hi:.2e}, "
                  f"half-width / s.e. {half / min(se_lo, se_hi):.3f}")
            if ref < 1e-3:
                left_out.append((t, name))
                continue
            assert 0 < lo <= hi and se_lo > 0 and se_hi > 0
            assert half < 0.25 * min(se_lo, se_hi), ("the edges are not fine enough for this run", t, name, half, se_lo, se_hi)
            assert lo - SIGMAS * se_lo <= ref <= hi + SIGMAS * se_hi, (tau, omega, albedo, t, name, lo, hi, ref, se_lo, se_hi)
    assert set(left_out) <= {(8.0, "fluxDown")}, left_out


# ---- 6: launches -----------------------------------------------------------------------------------------------------------------------
def test_tiny_and_split_batches_accumulation_and_zeroing():
    g = make_gpu(cases.step_cloud(ssa=0.97, nlayers=16, ncolumns=32), hg_table(), surfaceAlbedo=0.3, pathHistogramEdges=CLOUD_EDGES)
    for n in (1, 63):                                            # less than a wavefront: most lanes never hold a photon
        tiny = _run(g, n=n)
        c = tiny["counters"]
        assert c["photons"] == n and c["dropped"] == 0
        blk = _block(g, tiny)
        assert_same_sums(_one(blk["binUp"]), _one(_flux(g, tiny, "fluxUp")), c, what=("fluxUp", n))
        assert_same_sums(_one(blk["binDown"]), _one(_flux(g, tiny, "fluxDown")), c, what=("fluxDown", n))
        # (one photon may end in the roulette and tally nothing; of 63 some arrive)
        assert (n == 1 or blk["binUp"].sum() + blk["binDown"].sum() > 0) and all(blk[k][-1] == 0 for k in FIELDS)
    whole = _run(g)
    n1 = 12_345
    seq = M.new_RandomNumberSequence(SEED)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, n1), firstPhoton=0, zero=True)
    g.launch(seq, M.new_PhotonStream(*K.SOURCE, N - n1), firstPhoton=n1, zero=False)
    parts = g.finish()
    assert parts["counters"] == whole["counters"]
    assert_same_sums(parts["raw"], whole["raw"], whole["counters"], what="one launch against two")
    other = _run(g, seed=(SEED[0], SEED[1] + 1))
    g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N), zero=True)
    g.launch(M.new_RandomNumberSequence((SEED[0], SEED[1] + 1)), M.new_PhotonStream(*K.SOURCE, N), zero=False)
    both = g.finish()
    total = {k: whole["counters"][k] + other["counters"][k] for k in whole["counters"]}
    assert both["counters"] == total
    assert_same_sums(both["raw"], whole["raw"] + other["raw"], total, what="a second batch adds")
    _check_bins(g, both, CLOUD_EDGES, total)
    g._check(g._lib.i3rc_hip_zero_tallies(g._h), "zero_tallies")
    assert (g.fetch() == 0).all()
    g.finalize_Integrator()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    import torch

    d = cases.step_cloud(ssa=0.97, nlayers=8, ncolumns=16)
    edges = _geometric(2.5, 1.4, 80)
    fresh = make_gpu(d, hg_table(), surfaceAlbedo=0.3, pathHistogramEdges=edges)
    want = _run(fresh)
    fresh.finalize_Integrator()
    g = make_gpu(d, hg_table(), surfaceAlbedo=0.3)
    old_total = g.layout().total
    new_total = old_total + 4 * edges.size
    buf = torch.zeros(old_total, dtype=torch.float64, device="cuda")
    g.specifyParameters(pathHistogramEdges=edges)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) != 0     # the old length: too short now
    assert b"too small" in g._lib.i3rc_hip_last_error(g._h)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: the path histogram is tallied by flux launches only; radiance directions are set"):
        g.specifyParameters(intensityMus=[1.0], intensityPhis=[0.0])
        _run(g)
    g.specifyParameters(computeIntensity=False)
    # (from here on every refused call finds tallies in the buffer, and leaves them and the layout as they are)
    first = _run(g)
    layout = g.path_histogram_layout()
    assert layout[-1] == new_total and layout[-2] == 80

    def unchanged():
        assert g.path_histogram_layout() == layout and g.layout().total == new_total and np.array_equal(g.pathHistogramEdges, edges)
        assert np.array_equal(g.fetch(), first["raw"])

    # bad bins, each by what is wrong with it: the histogram stays on, with the bins it had
    for bad, text in ((np.zeros(1026, np.float32), "1 <= nBins <= 1024 required.*got 1025"),
                      (np.concatenate([[0.5], edges[1:]]), r"edges\[0\] must be 0"),
                      (np.concatenate([edges[:7], edges[5:7], edges[9:]]), r"edges must be strictly ascending; edges\[7\] is not above edges\[6\]"),
                      (np.concatenate([edges[:4], [np.nan], edges[5:]]), r"edges must be finite; edges\[4\] is not")):
        with pytest.raises(M.I3RCError, match="i3rc_hip_set_path_histogram: " + text):
            g.specifyParameters(pathHistogramEdges=bad)
        unchanged()
    g.specifyParameters(useRayTracing=False)
    with pytest.raises(M.I3RCError, match="i3rc_hip_launch_batch: the path histogram needs ray tracing; max cross-section is in use"):
        g.launch(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N), zero=False)
    with pytest.raises(M.I3RCError, match="i3rc_hip_compute_batch: the path histogram needs ray tracing; max cross-section is in use"):
        g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence(SEED), M.new_PhotonStream(*K.SOURCE, N))
    g.specifyParameters(useRayTracing=True)
    unchanged()
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches: the path histogram is tallied by plain launches only"):
        g.computeRadiativeTransferBatches(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_batches_moments: the path histogram is tallied by plain launches only"):
        g.computeRadiativeTransferBatchMoments(SEED, 3, *K.SOURCE, 1000)
    with pytest.raises(M.I3RCError, match="i3rc_hip_get_diagnostic_moments_layout: the path histogram has no batch statistics"):
        g.computeRadiativeTransferDiagnosticMoments(SEED, 3, *K.SOURCE, 1000)
    s, accepted = M.binding.Source(), C.c_int(7)
    s.kind, s.solarMu, s.solarAzimuth = 0, K.SOURCE[0], K.SOURCE[1]
    dummy = np.zeros(8 * new_total, np.float64)
    p = dummy.ctypes.data_as(M.binding.dp)
    assert g._lib.i3rc_hip_run_batches_diagnostic_moments(g._h, SEED[0], SEED[1], 3, 1000, C.byref(s), p, p, p, p, p) != 0
    assert b"i3rc_hip_run_batches_diagnostic_moments: the path histogram has no batch statistics" in g._lib.i3rc_hip_last_error(g._h)
    assert (dummy == 0).all()
    assert g._lib.i3rc_hip_expect_batches(g._h, SEED[0], SEED[1], 4, 1000, C.byref(s), C.byref(accepted)) != 0 and accepted.value == 0
    assert b"i3rc_hip_expect_batches: the path histogram is tallied by plain launches only" in g._lib.i3rc_hip_last_error(g._h)
    unchanged()
    # the blocks behind the counters share their place: none is switched on while another is
    for other, setter in (("computeLevelFluxes", "i3rc_hip_set_level_fluxes"), ("computeActinicFlux", "i3rc_hip_set_actinic_flux"),
                          ("computePathLengths", "i3rc_hip_set_path_lengths")):
        with pytest.raises(M.I3RCError, match=setter + ": the path histogram is switched on"):
            g.specifyParameters(**{other: True})
    assert g.level_flux_layout() == (-1, -1, new_total) and g.actinic_flux_layout() == (-1, new_total) and g.path_length_layout() == (-1, -1, -1, -1, new_total)
    unchanged()
    rng = np.random.default_rng(3)
    stream = M.PhotonStream(arrays=[rng.random(8), rng.random(8), np.full(8, 0.5), np.full(8, -0.7), np.zeros(8)])
    with pytest.raises(M.I3RCError, match="i3rc_hip_run_replay: the path histogram is tallied by the production stream's kernels only; the replay build has no such kernel"):
        g.run_replay(stream, rng.random(4096).astype(np.float32), np.arange(8) * 512)     # (the mirror clears the tallies before it asks)
    assert g.path_histogram_layout() == layout and g.layout().total == new_total
    # a normal launch afterwards: what a fresh handle gives; through i3rc_hip_compute_batch too (one launch per call, no look-ahead)
    got = _run(g)
    assert got["counters"] == want["counters"]
    assert_same_sums(got["raw"], want["raw"], want["counters"], what="after the refusals")
    for k in range(3):
        ahead = g.computeRadiativeTransferLookingAhead(M.new_RandomNumberSequence((SEED[0], SEED[1] + k)), M.new_PhotonStream(*K.SOURCE, N))
        assert "PhiloxBinStream" in g.kernel_name()
    again = _run(g, seed=(SEED[0], SEED[1] + 2))
    assert ahead["counters"] == again["counters"]
    assert_same_sums(ahead["raw"], again["raw"], again["counters"], what="compute_batch")
    g.specifyParameters(pathHistogramEdges=np.zeros(0, np.float32))
    assert g.layout().total == old_total and g.path_histogram_layout() == (-1, -1, -1, -1, 0, old_total) and g.pathHistogramEdges is None
    assert g._lib.i3rc_hip_normalise_path_histogram(g._h, dummy.ctypes.data_as(M.binding.dp), None, None, None, None) != 0
    assert b"i3rc_hip_normalise_path_histogram: the path histogram is not switched on" in g._lib.i3rc_hip_last_error(g._h)
    for other, text in (("computeLevelFluxes", "level fluxes are switched on"), ("computeActinicFlux", "the actinic flux is switched on"),
                        ("computePathLengths", "path lengths are switched on")):
        g.specifyParameters(**{other: True})
        with pytest.raises(M.I3RCError, match="i3rc_hip_set_path_histogram: " + text):
            g.specifyParameters(pathHistogramEdges=edges)
        g.specifyParameters(**{other: False})
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, C.c_void_p(buf.data_ptr()), C.c_size_t(old_total * 8)) == 0
    assert g._lib.i3rc_hip_set_path_histogram(g._h, 80, edges.ctypes.data_as(M.binding.fp)) != 0
    assert b"i3rc_hip_set_path_histogram: a caller-bound tally buffer is in use" in g._lib.i3rc_hip_last_error(g._h)
    assert g._lib.i3rc_hip_bind_tally_buffer(g._h, None, 0) == 0
    with pytest.raises(M.I3RCError, match="path histogram information not available"):
        _run(g)
        g.reportResults(pathHistogramUp=True)
    assert g.layout().total == old_total and g.pathHistogramEdges is None
    last = _run(g)
    assert "PhiloxBinStream" not in g.kernel_name() and last["counters"]["photons"] == N
    g.finalize_Integrator()


# ---- 8: the Fortran shell --------------------------------------------------------------------------------------------------------------
def test_shell_path_histogram_equals_the_python_mirror():
    from tests.test_fortran_shell import BUILD, _need, _run as run_exe

    exe = _need(os.path.join(BUILD, "pathHistogramTest"))
    r = run_exe([exe], cwd=ROOT)
    assert r.returncode == 0 and "pathHistogramTest done" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("unavailable  T reportResults: path histogram information not available") for l in lines), r.stdout
    assert any(l.startswith("badedges     T specifyParameters: i3rc_hip_set_path_histogram: edges must be strictly ascending; edges[4] is not above edges[3]") for l in lines), r.stdout
    assert any(l.startswith("exclusive    T specifyParameters: i3rc_hip_set_path_lengths: the path histogram is switched on") for l in lines), r.stdout
    assert any(l.startswith("wrongsize    T reportResults: pathHistogramPathDown array is the wrong size") for l in lines), r.stdout
    assert any(l.startswith("offagain     T") for l in lines), r.stdout
    nx, ny, nz, nbins = 4, 2, 6, 24
    ext = np.full((nz, ny, nx), f32(0.0002), np.float32)
    for k in range(2, 5):
        for j in range(ny):
            for i in range(nx):
                ext[k, j, i] = f32(0.004) * f32(1 + (i + 1 + j + 1) % 3)
    d = dict(xe=f32(500.0) * np.arange(nx + 1, dtype=np.float32), ye=f32(500.0) * np.arange(ny + 1, dtype=np.float32),
             ze=np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0, 1000.0], np.float32), ext=ext, ssa=np.full_like(ext, f32(0.95)),
             pf=np.ones(ext.shape, np.int32))
    edges = np.zeros(nbins + 1, np.float32)
    edges[1] = 500.0
    for b in range(2, nbins + 1):                                 # the shell's own float32 arithmetic: one product per edge
        edges[b] = edges[b - 1] * f32(1.25)
    g = make_gpu(d, hg_table(0.85, 64), surfaceAlbedo=0.3, minInverseTableSize=10001, pathHistogramEdges=edges)
    res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((7, 3)), M.new_PhotonStream(0.5, 30.0, 50_000))
    rep = g.reportResults(pathHistogramUp=True, pathHistogramPathUp=True, pathHistogramDown=True, pathHistogramPathDown=True)
    assert res["counters"]["photons"] == 50_000
    for tag, key in zip(("binUp", "binPathUp", "binDown", "binPathDown"), NAMES):
        row = [l.split() for l in lines if l.startswith(tag + " ")]
        assert len(row) == 1 and len(row[0]) == 1 + nbins + 1, row
        shell = np.array([float(v) for v in row[0][1:]])
        assert np.count_nonzero(rep[key]) > 8 and ((shell == 0) == (rep[key] == 0)).all(), (key, shell, rep[key])
        has = rep[key] != 0
        assert np.abs(shell[has] / rep[key].astype(np.float64)[has] - 1.0).max() <= 0.6e-8, (key, shell, rep[key])     # (nine digits are printed: the same float32)
    ratio = [l.split() for l in lines if l.startswith("ratioUp ")]
    assert len(ratio) == 1 and len(ratio[0]) == 4, ratio
    up, path = rep["pathHistogramUp"].astype(np.float64), rep["pathHistogramPathUp"].astype(np.float64)
    has = up > 0
    want = [np.sum(up[has] * np.exp(-float(f32(k)) * path[has] / up[has])) / up.sum() for k in (1e-5, 1e-4, 1e-3)]
    assert 0 < want[2] < want[1] < want[0] < 1
    assert np.abs(np.array([float(v) for v in ratio[0][1:]]) / np.array(want) - 1.0).max() <= 0.6e-12, (ratio, want)      # (thirteen digits)
    g.finalize_Integrator()
