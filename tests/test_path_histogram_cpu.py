"""The path-length histogram of reflected and transmitted light (i3rc_hip_set_path_histogram), the parts that need no GPU.

  layout          where the block's four fields lie and how long the buffer is, for three grids and two bin counts:
                  tests/path_histogram_main.cpp -- a host C++17 program over csrc/tally_block.hpp alone -- against the offsets restated
                  here; every other kind has no such block, and the path-length layout answers what it did
  normalisation   random raw blocks through the header's normalised_path_bin against float32(raw / photons) restated in float64
                  numpy, bit for bit
  bin rule        the header's path_bin -- the function the kernel calls -- against numpy.searchsorted(edges, x, side="right") - 1
                  clipped to nBins: on every edge, one float32 either side of it, between the edges, at 0 and beyond the last edge,
                  for nBins = 1, 2, 3, 64 and 1024; a NaN and a negative value stay inside the block
  plan            a histogram launch at all five places of the field, and on both sides of the LDS edge: the last field in LDS
                  beside which the region still fits the workgroup's budget, and the next, where the launch adds to global memory
                  instead of being refused
  symbols, ISA    the three entry points are declared, exported and bound; exactly five kernels, no spill, no scratch"""
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
NEW_SYMBOLS = ("i3rc_hip_set_path_histogram", "i3rc_hip_get_path_histogram_layout", "i3rc_hip_normalise_path_histogram")
PLACES = ("GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE")
HEADER_WORDS = 33
LDS_BUDGET = 64 * 1024               # csrc/launch_plan.hpp, kLdsBudget: what a workgroup may have where two are to share a compute unit

GRIDS = {"1 x 1 x 4": (1, 1, 4), "8 x 4 x 6": (8, 4, 6), "3 x 2 x 2": (3, 2, 2)}
BIN_COUNTS = (7, 1024)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("path_histogram") / "path_histogram_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "path_histogram_main.cpp")])
    return str(exe)


def restated_layout(nx, ny, nz, nbins):
    """i3rc_tally_layout of a flux problem with one component, the histogram's block behind the counters: four fields of nBins + 1 words"""
    ncol = nx * ny
    counters = 3 * ncol + ncol * nz                    # fluxUp, fluxDown, fluxAbsorbed, volumeAbsorption; no radiances
    block = counters + NUM_COUNTERS
    n = nbins + 1
    return dict(binUp=block, binPathUp=block + n, binDown=block + 2 * n, binPathDown=block + 3 * n, block=block, words=4 * n,
                counters=counters, total=block + 4 * n)


def run_layout(program, shape, nbins, tmp_path, seed=20250914):
    nx, ny, nz = shape
    lay = restated_layout(nx, ny, nz, nbins)
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.0, 5e4, lay["total"])
    raw[lay["counters"]:lay["counters"] + NUM_COUNTERS] = rng.integers(1, 1000, NUM_COUNTERS)
    raw[lay["counters"] + CNT_PHOTONS] = 100003.0
    raw[lay["binUp"] + 1] = 0.0                        # (an empty bin stays an exact zero)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nx, ny, nz, nbins], np.int64).tobytes())
        f.write(raw.tobytes())
    subprocess.check_call([program, "layout", str(src), str(dst)])
    header = np.fromfile(dst, np.int64, HEADER_WORDS).tolist()
    return lay, raw, header, np.fromfile(dst, np.float32, offset=8 * HEADER_WORDS)


@pytest.mark.parametrize("nbins", BIN_COUNTS)
@pytest.mark.parametrize("name", list(GRIDS))
def test_layout_of_the_block(program, name, nbins, tmp_path):
    nx, ny, nz = GRIDS[name]
    lay, _, header, _ = run_layout(program, GRIDS[name], nbins, tmp_path)
    names = ("binUp", "binPathUp", "binDown", "binPathDown", "block", "words", "counters", "total")
    assert dict(zip(names, header[:8])) == lay, (dict(zip(names, header[:8])), lay)
    ncol = nx * ny
    without = lay["counters"] + NUM_COUNTERS
    # none, levels, tracks: no path offsets, their own totals; path lengths: what they were -- four fields of nx ny words
    for k, words in enumerate((0, 2 * (nz + 1) * ncol, nz * ncol)):
        assert header[8 + 5 * k:13 + 5 * k] == [-1, -1, -1, -1, without + words], (k, header)
    assert header[23:28] == [without, without + ncol, without + 2 * ncol, without + 3 * ncol, without + 4 * ncol], header
    assert header[28:33] == [-1, -1, -1, -1, -1], header       # the histogram's own view: no path-length fields, no level fluxes


@pytest.mark.parametrize("nbins", BIN_COUNTS)
@pytest.mark.parametrize("name", list(GRIDS))
def test_normalisation_is_per_photon_of_the_block_bit_for_bit(program, name, nbins, tmp_path):
    lay, raw, _, got = run_layout(program, GRIDS[name], nbins, tmp_path)
    want = np.float32(raw[lay["block"]:lay["block"] + lay["words"]] / raw[lay["counters"] + CNT_PHOTONS])
    assert got.shape == want.shape and np.all(np.isfinite(want)) and want[1] == 0.0 and np.count_nonzero(want) == want.size - 1
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, (name, differ[:8], got[differ[:8]], want[differ[:8]])


def _edges(nbins):
    """float32 edges from 0 in geometric progression, strictly ascending (a ratio the float32 spacing resolves at every edge)"""
    e = np.concatenate([[0.0], 0.01 * np.float64(1.0 + 8.0 / max(nbins, 8)) ** np.arange(nbins)]).astype(np.float32)
    assert e.size == nbins + 1 and np.all(np.diff(e) > 0) and np.all(np.isfinite(e))
    return e


@pytest.mark.parametrize("nbins", (1, 2, 3, 64, 1024))
def test_bin_rule_against_searchsorted(program, nbins, tmp_path):
    e = _edges(nbins)
    inf = np.float32(np.inf)
    x = np.concatenate([e, np.nextafter(e, -inf), np.nextafter(e, inf), np.float32(0.5) * (e[1:] + e[:-1]),
                        np.float32([0.0, 2.0 * e[-1], 1e30, np.finfo(np.float32).max, inf])]).astype(np.float32)
    x = x[x >= 0]                                          # (one float32 below edges[0] = 0 is negative: see below)
    want = np.clip(np.searchsorted(e, x, side="right") - 1, 0, nbins).astype(np.int32)
    assert want.min() == 0 and want.max() == nbins and set(want.tolist()) == set(range(nbins + 1))
    odd = np.float32([np.nan, -1.0, -0.0, -inf])          # no path has these: whatever the rule answers lies inside the block
    src, dst = tmp_path / "bins_in.bin", tmp_path / "bins_out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nbins, x.size + odd.size], np.int64).tobytes())
        f.write(e.tobytes()); f.write(x.tobytes()); f.write(odd.tobytes())
    subprocess.check_call([program, "bins", str(src), str(dst)])
    got = np.fromfile(dst, np.int32)
    assert got.size == x.size + odd.size
    differ = np.flatnonzero(got[:x.size] != want)
    assert differ.size == 0, (nbins, differ[:8], x[differ[:8]], got[differ[:8]], want[differ[:8]])
    assert np.all((got[x.size:] >= 0) & (got[x.size:] <= nbins)) and got[x.size + 2] == 0, got[x.size:]


# ---- the launch plan -----------------------------------------------------------------------------------------------------------------
def _plans(d, tabs, row, nbins, lds_tallies=None):
    """(name, plan) of a histogram launch and of a path-length launch on the same facts and knobs"""
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    lds = row["lds_tallies"] if lds_tallies is None else lds_tallies
    setup = S.setup(S.PARAMS[row["params"]], tabs[0].n_entries, row["inv"], "level", row["kernel"], row["place"], lds, row["surface"])
    facts = S.facts(d)
    bins = B.plan_launch(facts, dict(setup, extra=B.EXTRA_KINDS["bins"]), stream="bins", source=row["src"], path_bins=nbins)
    path = B.plan_launch(facts, dict(setup, extra=B.EXTRA_KINDS["paths"]), stream="path", source=row["src"])
    return bins, path


def _region_bytes(nbins):
    return 4 * (nbins + 1) * 8 + (nbins + 1) * 4          # four fields of float64 sums, the float32 edges behind them


def test_a_histogram_launch_at_all_five_places():
    """the path-length launch's plan in everything but the kernel's name, the region behind the plan's end where the sums lie in LDS,
    and the word that says so"""
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    rows = [S._row(f"{dom}/bins/{place}", spec, "flux", kind="level", place=place)
            for dom, spec, place in (("step", ("matrix", "step"), "auto"), ("two", ("matrix", "two"), "linear"), ("wide", ("wide", 342, 9, 1), "auto"),
                                     ("columns2", ("matrix", "columns2"), "columns"), ("colbase2", ("matrix", "colbase2"), "columns"))]
    places = set()
    for row in rows:
        d, tabs = S.domain(row["domain"])
        for nbins in (64, 1024):
            for lds in (True, False):
                (name_b, plan_b), (name_p, plan_p) = _plans(d, tabs, row, nbins, lds)
                assert plan_b is not None and plan_p is not None, (row["id"], name_b, name_p)
                assert name_b == name_p.replace("PhiloxPathStream", "PhiloxBinStream") and name_b.startswith("photon_kernel<PhiloxBinStream, false, true, GRID_"), name_b
                in_lds = plan_b.pop(B.PLAN_BIN_NAME)
                assert in_lds == int(lds), (row["id"], nbins, lds, plan_b)      # (these fields leave room at every place)
                grown = plan_b["ldsBytes"] - plan_p["ldsBytes"]
                # (the region begins at the next 8-byte boundary behind the plan's end and the allocation is rounded up to 16 bytes)
                assert (_region_bytes(nbins) - 12 <= grown <= _region_bytes(nbins) + 16) if lds else grown == 0, (row["id"], nbins, grown)
                assert dict(plan_b, ldsBytes=0) == dict(plan_p, ldsBytes=0), (row["id"], plan_b, plan_p)
                assert plan_b["ldsTrackSums"] == 0 and plan_b["startStoreBytes"] == 0 and plan_b["tableInLds"] == 0 and plan_b["threads"] == 256, plan_b
        places.add(name_b.split(", ")[-1])
    assert places == {p + ">" for p in PLACES}, places


def test_both_sides_of_the_lds_edge():
    """A conservative 1 x 1 column keeps its field in LDS; a layer more is two floats more of it (an edge and a cell).  1024 bins: the
    region is 36 900 bytes.  At the last nz at which the launch with the region stays within the budget of a workgroup the sums lie in
    LDS and the allocation is that budget less than one layer's step; one layer more and the launch is planned all the same -- same
    kernel, same place, the allocation the path-length launch's -- with the sums in global memory."""
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S
    from tests import test_gpu_limits as L

    nbins = 1024
    row = S._row("column/bins", ("column",), "flux", kind="level")
    tabs = [S._hg(0.85)]

    def plans(nz):
        return _plans(L._column(nz, ncomp=1, ssa=1.0), tabs, row, nbins)

    lo, hi = 2000, 5000
    assert plans(lo)[0][1][B.PLAN_BIN_NAME] == 1 and plans(hi)[0][1][B.PLAN_BIN_NAME] == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plans(mid)[0][1][B.PLAN_BIN_NAME] == 1 else (lo, mid)
    (name_in, plan_in), (_, path_in) = plans(lo)
    (name_out, plan_out), (name_path, path_out) = plans(hi)
    print("last nz with the sums in LDS", lo, plan_in["ldsBytes"], "bytes; then", plan_out["ldsBytes"], "bytes")
    assert plan_in["ldsGrid"] == 1 and plan_out["ldsGrid"] == 1 and plan_in["place"] == 0 and plan_out["place"] == 0
    assert plan_in[B.PLAN_BIN_NAME] == 1 and LDS_BUDGET - 16 < plan_in["ldsBytes"] <= LDS_BUDGET, plan_in
    assert _region_bytes(nbins) - 12 <= plan_in["ldsBytes"] - path_in["ldsBytes"] <= _region_bytes(nbins) + 16, (plan_in, path_in)   # (alignment and rounding)
    assert plan_out[B.PLAN_BIN_NAME] == 0 and plan_out["ldsBytes"] == path_out["ldsBytes"], (plan_out, path_out)
    assert path_out["ldsBytes"] + _region_bytes(nbins) > LDS_BUDGET
    assert name_out == name_in == "photon_kernel<PhiloxBinStream, false, true, GRID_LDS>" and name_path == name_in.replace("Bin", "Path")


def test_refusals_of_a_plan_are_the_path_length_plan_s():
    from i3rc_monte_carlo_model_amd import binding as B
    from tests import plan_sweep as S

    d, tabs = S.domain(("matrix", "step"))
    setup = dict(S.setup(S.PARAMS["flux"], tabs[0].n_entries, S.SMALL_INV, "level"), inverseTables=0)
    text_p, plan_p = B.plan_launch(S.facts(d), dict(setup, extra=B.EXTRA_KINDS["paths"]), stream="path")
    text_b, plan_b = B.plan_launch(S.facts(d), dict(setup, extra=B.EXTRA_KINDS["bins"]), stream="bins", path_bins=16)
    assert plan_p is None and plan_b is None and text_b == text_p and "inverse phase function table missing" in text_b, (text_p, text_b)
    for bad in (0, 1025):
        with pytest.raises(M.I3RCError, match="bad arguments"):
            B.plan_launch(S.facts(d), dict(setup, extra=B.EXTRA_KINDS["bins"]), stream="bins", path_bins=bad)


def test_the_diagnostic_moments_layout_has_no_slot_for_the_kind():
    with pytest.raises(M.I3RCError, match="bad arguments"):
        M.binding.diagnostic_moments_layout("bins", 3, 2, 2)


def test_path_histogram_symbols_are_exported_and_bound():
    lib = M.binding.load()
    header = open(os.path.join(ROOT, "include", "i3rc_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in M.binding.SYMBOLS, name
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name
    assert M.binding.STREAM_KINDS["bins"] == 6 and M.binding.EXTRA_KINDS["bins"] == 4 and M.binding.MAX_PATH_BINS == 1024
    assert M.binding.PLAN_BIN_NAME not in M.binding.PLAN_NAMES and len(M.binding.PLAN_NAMES) == 13


def test_path_histogram_kernels_keep_their_state_in_registers():
    """exactly the five instantiations -- whose names no earlier audit counts --, no spilled vector register, no scratch"""
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources

    rows = [r for r in resources() if "PhiloxBinStream" in r["name"]]
    assert sorted(r["name"] for r in rows) == sorted(f"photon_kernel<PhiloxBinStream, false, true, {p}>" for p in PLACES), [r["name"] for r in rows]
    for r in rows:
        assert "PhiloxPathStream" not in r["name"] and "<PhiloxStream," not in r["name"] and "<PhiloxBatchStream," not in r["name"]
        print(r["name"], "VGPRs", r["VGPRs"], "SGPR spills", r["SGPRs Spill"], "occupancy", r["Occupancy [waves/SIMD]"])
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (r["name"], r["VGPRs Spill"], r["ScratchSize [bytes/lane]"])
