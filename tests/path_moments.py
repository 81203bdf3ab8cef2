"""What the two suites of the path moments share (tests/test_path_moments_cpu.py, tests/test_gpu_path_moments.py): the float64 numpy
restatement of what a batch adds to them (csrc/tally_block.hpp: path_moments_layout, domain_path_ratio, path_spectrum_term), from a
batch's raw block.  Every sum is taken in the order of its elements.  A plain module beside tests/extra_tally.py."""
import numpy as np

PATHS, BINS = 3, 4                   # csrc/tally_block.hpp, ExtraTally
SCALARS = ("meanPathLengthUp", "meanPathLengthSquaredUp", "meanPathLengthDown", "meanPathLengthSquaredDown",
           "domainPathUp", "domainPathSquaredUp", "domainPathDown", "domainPathSquaredDown")
SPECTRUM = ("spectrumUpLower", "spectrumUpUpper", "spectrumDownLower", "spectrumDownUpper")


def restated_layout(kind, nx, ny, nbins=0, nk=0):
    """the words of i3rc_path_moments_layout behind nK, by name: contiguous in the stated order, -1 what the kind has not"""
    names = ["pathLengthUp", "pathLengthSquaredUp", "pathLengthDown", "pathLengthSquaredDown", *SCALARS,
             "histogramUp", "histogramPathUp", "histogramDown", "histogramPathDown", *SPECTRUM]
    o, at, ncol = dict.fromkeys(names, -1), 0, nx * ny
    parts = {PATHS: [(n, ncol) for n in names[:4]] + [(n, 1) for n in SCALARS],
             BINS: [(n, nbins + 1) for n in names[12:16]] + [(n, nk) for n in SPECTRUM]}.get(kind, [])
    for name, n in parts:
        o[name], at = at, at + n
    o["total"] = at
    return o


def seq_sum(x):
    """the float64 sum of x in the order of its elements (numpy's own sum is pairwise)"""
    total = 0.0
    for v in np.asarray(x, np.float64).ravel():
        total += float(v)
    return total


def domain_ratios(path_fields, flux_up, flux_down):
    """float32(sum of the raw path field / sum of the raw flux), 0 where the flux is 0: path_fields = (pathUp1, pathUp2, pathDown1,
    pathDown2), raw; in SCALARS[4:]'s order"""
    out = []
    for f, field in enumerate(path_fields):
        den = seq_sum(flux_up if f < 2 else flux_down)
        out.append(np.float32(seq_sum(field) / den) if den > 0 else np.float32(0))
    return np.array(out, np.float32)


def spectrum_terms(weight, path, edges, k):
    """per bin (the overflow bin last) the lower and the upper term of sum_b u_b <exp(-k L)>_b, float64: weight, path the raw fields of
    nBins + 1 words, edges the float32 edges, k one coefficient (a float32 value)"""
    u, p, e, k = np.asarray(weight, np.float64), np.asarray(path, np.float64), np.asarray(edges, np.float32).astype(np.float64), float(np.float32(k))
    nb = e.size - 1
    has = u > 0
    with np.errstate(all="ignore"):
        m = np.where(has, p / np.where(has, u, 1.0), 0.0)
    e0, e1 = e[:-1], e[1:]
    mb = np.minimum(np.maximum(m[:nb], e0), e1)
    lower = u[:nb] * np.exp(-k * mb)
    upper = (u[:nb] * ((e1 - mb) * np.exp(-k * e0) + (mb - e0) * np.exp(-k * e1))) / (e1 - e0)
    mo = max(m[nb], e[nb])
    lower = np.append(np.where(has[:nb], lower, 0.0), u[nb] * np.exp(-k * mo) if has[nb] else 0.0)
    upper = np.append(np.where(has[:nb], upper, 0.0), u[nb] * np.exp(-k * e[nb]) if has[nb] else 0.0)
    return lower, upper


def spectrum_bounds(weight, path, edges, ks, photons):
    """(lower[nK], upper[nK]) in float64, not yet rounded: the sums of spectrum_terms over the bins, per photon"""
    lo, hi = [], []
    for k in ks:
        lower, upper = spectrum_terms(weight, path, edges, k)
        lo.append(seq_sum(lower) / photons)
        hi.append(seq_sum(upper) / photons)
    return np.array(lo), np.array(hi)
