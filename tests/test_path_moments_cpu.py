"""The path moments without a GPU: where they lie (csrc/tally_block.hpp, path_moments_layout, through the host-only
i3rc_hip_path_moments_layout_words), and what a batch adds to them (normalised_extra_value, domain_path_ratio, path_spectrum_term,
through tests/path_moments_main.cpp -- a host C++17 program over that header alone, built with -ffp-contract=off as the library is).

Layout: restated in tests/path_moments.py and compared word for word.

Values: every word of a random raw block against a float64 numpy restatement rounded once to float32.  Fields, means and domain ratios
are divisions and sums in the order of their elements: bit for bit.  A spectrum word holds libm's exp against numpy's: both are
within an ulp of float64, far inside the one float32 ulp allowed.

Conditions of tests/test_gpu_path_moments.py::test_the_spectrum_brackets_the_adding_solver, which leaves nothing out: no reference
ratio of its four slabs at its three absorber depths is below 1e-3 (the batch means of exp(-k L) are not Gaussian below that:
tests/test_gpu_path_histogram.py).  All three values of TAU_A pass; none had to be dropped."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M
from tests import path_moments as P

B = M.binding
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i3rc-monte-carlo-model_amd", "csrc")
NUM_COUNTERS, CNT_PHOTONS = 16, 0    # include/i3rc_hip.h
PATHS, BINS = P.PATHS, P.BINS
TAU_A = (0.05, 0.5, 2.0)
SLABS = [(tau, omega, albedo) for tau in (1.0, 10.0) for omega, albedo in ((0.9, 0.5), (1.0, 0.0))]


# ---- the layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (8, 4), (3, 40443)], ids=["1x1", "8x4", "3x40443"])
def test_paths_layout_is_contiguous_in_the_stated_order(size):
    nx, ny = size
    got = B.path_moments_layout(PATHS, nx, ny)
    assert got == P.restated_layout(PATHS, nx, ny), got
    assert got["total"] == 4 * nx * ny + 8 and got["domainPathSquaredDown"] == got["total"] - 1
    assert B.path_moments_layout("paths", nx, ny, 5, 9) == got          # (neither bins nor coefficients size this kind)
    assert list(got) == B.PATH_MOMENTS_NAMES


@pytest.mark.parametrize("bins", [(1, 0), (7, 3), (1024, 256)], ids=["1+0", "7+3", "1024+256"])
def test_bins_layout_is_contiguous_in_the_stated_order(bins):
    nbins, nk = bins
    got = B.path_moments_layout(BINS, 8, 4, nbins, nk)
    assert got == P.restated_layout(BINS, 8, 4, nbins, nk), got
    assert got["total"] == 4 * (nbins + 1) + 4 * nk
    assert B.path_moments_layout("bins", 1, 1, nbins, nk) == got       # (nor does the grid size this one)


def test_layout_refuses_bad_arguments():
    lib, out = B.load(), (B.C.c_int64 * 21)()
    words = lib.i3rc_hip_path_moments_layout_words
    assert words(PATHS, 8, 4, 0, 0, out, 21) == 0 and words(BINS, 8, 4, 7, 3, out, 21) == 0
    for kind in (-1, 0, 1, 2, 5):
        assert words(kind, 8, 4, 7, 3, out, 21) != 0, kind
    assert words(PATHS, 0, 4, 0, 0, out, 21) != 0 and words(PATHS, 8, 0, 0, 0, out, 21) != 0      # a size below 1
    assert words(BINS, 8, 4, 0, 3, out, 21) != 0 and words(BINS, 8, 4, 1025, 3, out, 21) != 0     # nBins outside 1 ... 1024
    assert words(BINS, 8, 4, 1024, 256, out, 21) == 0
    assert words(BINS, 8, 4, 7, -1, out, 21) != 0 and words(BINS, 8, 4, 7, 257, out, 21) != 0      # nK outside 0 ... 256
    assert words(PATHS, 8, 4, 0, 257, out, 21) != 0
    assert words(PATHS, 8, 4, 0, 0, None, 21) != 0
    assert words(PATHS, 8, 4, 0, 0, out, 20) != 0                                                 # a short answer
    with pytest.raises(M.I3RCError, match="i3rc_hip_path_moments_layout_words"):
        B.path_moments_layout(PATHS, 8, 4, nout=3)


def test_symbols_and_mirror():
    lib = B.load()
    header = open(os.path.join(ROOT, "include", "i3rc_hip.h")).read()
    for name in ("i3rc_hip_set_path_spectrum", "i3rc_hip_get_path_moments_layout", "i3rc_hip_path_moments_layout_words", "i3rc_hip_run_batches_path_moments"):
        assert name in B.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
    assert "typedef struct i3rc_path_moments_layout" in header
    assert [k for k, _ in B.PathMomentsLayout._fields_] == ["kind", "nBins", "nK"] + B.PATH_MOMENTS_NAMES
    assert all(k in header for k in B.PATH_MOMENTS_NAMES)
    assert callable(getattr(M.host.Integrator, "computeRadiativeTransferPathMoments"))
    assert "absorptionCoefficients" in M.host.Integrator._PARAM_KEYS


# ---- the values ---------------------------------------------------------------------------------------------------------------------------
GRID = dict(xe=[0.0, 10.0, 25.0, 31.0], ye=[-3.0, 4.5, 9.0], ze=[0.0, 0.3, 2.0, 2.5, 7.0])      # 3 x 2 x 4, every spacing unequal


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("path_moments") / "path_moments_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "path_moments_main.cpp")])
    return str(exe)


def _evaluate(program, tmp_path, kind, regular, raw, edges=(), ks=()):
    xe, ye, ze = (np.float32(GRID[k]) for k in ("xe", "ye", "ze"))
    nx, ny, nz = len(xe) - 1, len(ye) - 1, len(ze) - 1
    nbins = max(len(edges) - 1, 0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nx, ny, nz, regular, kind, nbins, len(ks)], np.int64).tobytes())
        for e in (xe, ye, ze, np.float32(edges), np.float32(ks)):
            f.write(e.tobytes())
        f.write(raw.tobytes())
    subprocess.check_call([program, str(src), str(dst)])
    header = np.fromfile(dst, np.int64, 22)
    lay = dict(zip(B.PATH_MOMENTS_NAMES, header[1:].tolist()))
    assert lay == P.restated_layout(kind, nx, ny, nbins, len(ks)) == B.path_moments_layout(kind, nx, ny, nbins, len(ks))
    got = np.fromfile(dst, np.float32, offset=header.nbytes)
    assert got.size == lay["total"]
    return int(header[0]), lay, got


def _raw_block(kind, words, seed):
    """a random raw block of the 3 x 2 x 4 grid (one component, no directions) with `words` of the kind behind the counters"""
    ncol, nz = 6, 4
    counters = 3 * ncol + ncol * nz
    block = counters + NUM_COUNTERS
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.5, 50.0, block + words)
    raw[counters:block] = rng.integers(1, 1000, NUM_COUNTERS)
    raw[counters + CNT_PHOTONS] = 4321.0
    return raw, counters, block, rng


def _same_bits(a, b, what):
    a, b = np.atleast_1d(np.float32(a)), np.atleast_1d(np.float32(b))
    differ = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    assert differ.size == 0, (what, differ[:8], a[differ[:8]], b[differ[:8]])


@pytest.mark.parametrize("regular", [0, 1], ids=["irregular", "declared regular"])
def test_path_length_words_of_a_batch(program, regular, tmp_path):
    nx, ny, ncol = 3, 2, 6
    raw, counters, block, _ = _raw_block(PATHS, 4 * ncol, 20261020 + regular)
    at, lay, got = _evaluate(program, tmp_path, PATHS, regular, raw)
    assert at == block
    x64, y64 = np.float64(np.float32(GRID["xe"])), np.float64(np.float32(GRID["ye"]))
    if regular:
        per_col = np.full((ny, nx), raw[counters + CNT_PHOTONS] / float(ncol))
    else:
        per_col = ((y64[1:] - y64[:-1])[:, None] * (x64[1:] - x64[:-1])[None, :]) / ((x64[-1] - x64[0]) * (y64[-1] - y64[0])) * raw[counters + CNT_PHOTONS]
    fields = np.float32(raw[block:].reshape(4, ny, nx) / per_col[None])
    assert np.all(fields > 0) and len(np.unique(fields)) > 12
    _same_bits(got[:4 * ncol], fields.ravel(), "fields")
    means = [np.float32(P.seq_sum(fields[f]) / float(ncol)) for f in range(4)]
    _same_bits(got[lay["meanPathLengthUp"]:lay["meanPathLengthUp"] + 4], means, "means")
    ratios = P.domain_ratios(raw[block:].reshape(4, ncol), raw[0:ncol], raw[ncol:2 * ncol])
    assert np.all(ratios > 0)
    _same_bits(got[lay["domainPathUp"]:lay["domainPathUp"] + 4], ratios, "domain ratios")


def test_a_domain_without_reflected_light_has_ratio_zero(program, tmp_path):
    raw, counters, block, _ = _raw_block(PATHS, 24, 7)
    raw[0:6] = 0.0                    # fluxUp
    at, lay, got = _evaluate(program, tmp_path, PATHS, 0, raw)
    assert got[lay["domainPathUp"]] == 0 and got[lay["domainPathSquaredUp"]] == 0 and got[lay["domainPathDown"]] > 0


EDGES = np.array([0.0, 0.5, 1.25, 2.0, 3.5, 6.0, 10.0, 17.0], np.float32)      # 7 bins
KS = np.array([0.0, 0.3, 40.0], np.float32)


def _histogram_block(seed=11):
    nb = EDGES.size
    raw, counters, block, rng = _raw_block(BINS, 4 * nb, seed)
    e = EDGES.astype(np.float64)
    for f in (0, 2):
        u = rng.uniform(5.0, 400.0, nb)
        frac = rng.uniform(0.05, 0.95, nb)
        m = np.append(e[:-1] + frac[:-1] * (e[1:] - e[:-1]), e[-1] * (1.0 + frac[-1]))      # (a filled overflow bin: its mean path beyond the last edge)
        u[3] = 0.0                                                                            # an empty bin
        m[5] = e[5]                                                                           # a mean path on its bin's lower edge
        raw[block + f * nb:block + (f + 1) * nb] = u
        raw[block + (f + 1) * nb:block + (f + 2) * nb] = u * m
    assert raw[block + nb - 1] > 0 and raw[block + 3] == 0 and raw[block + nb + 5] == raw[block + 5] * e[5]
    return raw, counters, block


def test_histogram_words_of_a_batch(program, tmp_path):
    from tests.test_gpu_path_histogram import _bracket

    nb = EDGES.size
    raw, counters, block = _histogram_block()
    photons = raw[counters + CNT_PHOTONS]
    at, lay, got = _evaluate(program, tmp_path, BINS, 0, raw, EDGES, KS)
    assert at == block
    _same_bits(got[:4 * nb], np.float32(raw[block:block + 4 * nb] / photons), "fields")
    for d, (lo_name, hi_name) in enumerate((("spectrumUpLower", "spectrumUpUpper"), ("spectrumDownLower", "spectrumDownUpper"))):
        u, p = raw[block + 2 * d * nb:block + (2 * d + 1) * nb], raw[block + (2 * d + 1) * nb:block + (2 * d + 2) * nb]
        lower, upper = P.spectrum_bounds(u, p, EDGES, KS, photons)
        for name, want in ((lo_name, lower), (hi_name, upper)):
            g = got[lay[name]:lay[name] + KS.size].astype(np.float64)
            w = np.float32(want).astype(np.float64)
            print(name, "program", g, "restatement", w, "difference in float32 ulps", np.abs(g - w) / np.spacing(np.float32(want)))
            assert np.all(np.abs(g - w) <= np.spacing(np.float32(want)).astype(np.float64)), (name, g, w)
        lo32, hi32 = got[lay[lo_name]:lay[lo_name] + KS.size], got[lay[hi_name]:lay[hi_name] + KS.size]
        assert np.all(lo32 <= hi32) and np.all(lower <= upper), (lo32, hi32)
        assert lo32[1] < hi32[1] and lo32[2] < hi32[2]                    # (k > 0: the chord lies above the curve)
        # k = 0: the sum of the bins over the photons, in both bounds -- the domain's mean flux
        _same_bits([lo32[0], hi32[0]], [np.float32(P.seq_sum(u) / photons)] * 2, "k = 0")
        # ... and the upper bound is the existing bracket's, which works from the normalised histogram (here: unrounded shares)
        for j, k in enumerate(KS):
            _, bracket_upper = _bracket(u / photons, p / photons, EDGES, float(k))
            assert abs(bracket_upper * P.seq_sum(u / photons) - upper[j]) <= 1e-13 * upper[j], (k, bracket_upper, upper[j])


def test_the_terms_of_the_special_bins():
    """the restatement itself, bin by bin: an empty bin adds nothing; a mean path on the lower edge makes the chord meet the curve;
    the overflow bin's upper term is its weight at its edge"""
    nb = EDGES.size
    raw, counters, block = _histogram_block()
    u, p = raw[block:block + nb], raw[block + nb:block + 2 * nb]
    lower, upper = P.spectrum_terms(u, p, EDGES, 0.3)
    assert lower[3] == 0 and upper[3] == 0
    assert lower[5] == upper[5] == u[5] * np.exp(-float(np.float32(0.3)) * float(EDGES[5]))
    assert upper[7] == u[7] * np.exp(-float(np.float32(0.3)) * float(EDGES[7])) and 0 < lower[7] < upper[7]
    assert np.all(lower <= upper)


# ---- what the GPU statistics test relies on -------------------------------------------------------------------------------------------------
def test_no_reference_ratio_of_the_statistics_test_is_below_a_thousandth():
    from tests.test_gpu_path_histogram import _solver_ratios

    for tau, omega, albedo in SLABS:
        ratios = _solver_ratios(tau, omega, albedo)
        for t in TAU_A:
            print("tau", tau, "omega", omega, "albedo", albedo, "tau_a", t, "ratios (up, down)", ratios[t])
            assert np.all(ratios[t] >= 1e-3), (tau, omega, albedo, t, ratios[t])
