// One raw tally block -- where its fields lie, and the rule that turns its float64 sums into the real(4) fields reportResults
// hands out (computeRadiativeTransfer :327-395) -- stated once for the host (i3rc_hip_normalise, i3rc_hip_normalise_level_fluxes, i3rc_hip_normalise_actinic_flux)
// and for the kernels (the batch moments).  The library is built with -ffp-contract=off, so both sides round alike.
// Plain C++17: no HIP header is needed (a host compiler alone builds tests/normalise_main.cpp against it).
#pragma once

#include <cmath>

#include "../../include/i3rc_hip.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define I3RC_TALLY_FN __host__ __device__ __forceinline__
#else
#define I3RC_TALLY_FN inline
#endif

namespace i3rc {

// Passed by value, also as a kernel argument; the two arrays are host memory on the host and device memory in a kernel.
struct TallyView {
  // offsets in float64 elements (tally_layout below; the level block lies behind the counters, -1 while it is switched off)
  long long fluxUp, fluxDown, fluxAbsorbed, volumeAbsorption, intensityByComponent, intensityExcess, counters, levelUp, levelDown;
  long long pathUp1, pathUp2, pathDown1, pathDown2;   // the path-length block's four fields, [ny][nx] each (-1 unless the block is EXTRA_PATHS)
  long long radiancePath1, radiancePath2;             // the radiance path block's two fields, [nDir][ny][nx] each (-1 unless the block is EXTRA_RADIANCE_PATHS)
  int nx, ny, nz, ncomp, nDir, xyRegular;
  int limitContrib;         // the excess of limited radiance contributions is redistributed (:327-347)
  const double *areaFrac;   // [nx * ny] column area / domain area (:358-366; read on irregular grids only)
  const double *dz;         // [nz] layer depths (:378-381)
};

// THE OPTIONAL DIAGNOSTIC TALLY: at most one more block, behind the counters of the packed tally buffer, that the general flux kernel of
// a plain, traced launch fills under a tag type of the production stream (philox.hpp, kExtra).  Which one is on is one value, on the
// handle and in the kernels alike; the kinds are never on together, so the block of either begins at the same word.
enum ExtraTally {
  EXTRA_NONE,
  EXTRA_LEVELS,   // levelFluxUp | levelFluxDown, [nz + 1][ny][nx] each (i3rc_hip_set_level_fluxes)
  EXTRA_TRACKS,   // the actinic flux's track-length sums, [nz][ny][nx] (i3rc_hip_set_actinic_flux)
  EXTRA_PATHS,    // pathUp1 | pathUp2 | pathDown1 | pathDown2, [ny][nx] each: the sums of w L and w L^2 over the photons that fluxUp / fluxDown count,
                  // L the geometric path since the photon's start (i3rc_hip_set_path_lengths)
  EXTRA_PATH_BINS, // binUp | binPathUp | binDown | binPathDown, nBins + 1 words each, domain-wide: the sums of w and of w L over the same photons, by the
                  // bin of L (path_bin below; the last word of each field is the overflow bin) (i3rc_hip_set_path_histogram)
  EXTRA_RADIANCE_PATHS   // radiancePath1 | radiancePath2, [nDir][ny][nx] each: the sums of c L and c L^2 over the contributions c that a launch adds to
                  // the radiance of a direction and column, summed over the components -- L the photon's geometric path up to the event plus
                  // the local-estimate ray's length to the top of the domain (i3rc_hip_set_radiance_path_lengths).  The one kind that the
                  // general RADIANCE kernel fills, and whose block is sized by nDir (radiance_path_block_words)
};
constexpr int kMaxPathBins = 1024;   // (i3rc_hip_set_path_histogram: 1 <= nBins <= 1024)
I3RC_TALLY_FN long long extra_block_offset(long long countersOffset) { return countersOffset + I3RC_NUM_COUNTERS; }
// ... and its length in float64 words (of the kinds the grid sizes: the path histogram's block is sized by its bins, path_bin_block_words)
// (... and the radiance path block by the directions)
I3RC_TALLY_FN long long radiance_path_block_words(int nDir, int nx, int ny) { return 2 * (long long)nDir * nx * ny; }
I3RC_TALLY_FN long long extra_block_words(ExtraTally kind, int nx, int ny, int nz) {
  const long long ncol = (long long)nx * ny;
  return kind == EXTRA_LEVELS ? 2 * (nz + 1) * ncol : (kind == EXTRA_TRACKS ? ncol * nz : (kind == EXTRA_PATHS ? 4 * ncol : 0));
}

// THE PATH HISTOGRAM (EXTRA_PATH_BINS): nBins bins over nBins + 1 float32 edges -- edges[0] == 0, strictly ascending, finite -- and an
// overflow bin behind them.  THE BIN RULE, for the host's tests and the kernel alike: a path L belongs to the bin b with
// edges[b] <= float(L) < edges[b + 1], and to the overflow bin b = nBins where float(L) >= edges[nBins].  The search makes
// ceil(log2(nBins + 1)) steps whatever L is -- no exit that depends on the data --, reads no edge beyond edges[nBins], and its answer is
// clamped to 0 ... nBins, so that nothing is written outside the block (a NaN or a negative L falls into bin 0).
// Edges: anything indexable that yields float (a host array, device memory, a pointer into LDS).
template <class Edges>
I3RC_TALLY_FN int path_bin(Edges edges, int nBins, float x) {
  int trips = 0;
  while ((nBins >> trips) != 0) ++trips;   // (the bits of nBins = ceil(log2(nBins + 1)))
  int b = 0;
  for (int k = trips - 1; k >= 0; --k) {
    const int c = b + (1 << k);
    const int at = c < nBins ? c : nBins;
    const bool take = (c <= nBins) & (edges[at] <= x);
    b = take ? c : b;
  }
  return b < 0 ? 0 : (b > nBins ? nBins : b);
}
// ... the block's length in float64 words, ...
I3RC_TALLY_FN long long path_bin_block_words(int nBins) { return 4 * ((long long)nBins + 1); }
// ... where the block's four fields begin (relative to the block), in float64 words: field 0 binUp, 1 binPathUp, 2 binDown, 3 binPathDown
I3RC_TALLY_FN long long path_bin_field(int field, int nBins) { return (long long)field * ((long long)nBins + 1); }
// ... and a word of the block as reportResults hands it out: per photon of the launch, domain-wide (so that the sum over binUp is the
// domain's area-weighted mean fluxUp on every grid)
I3RC_TALLY_FN float normalised_path_bin(const double *raw, long long countersOffset, long long at) {
  return (float)(raw[at] / raw[countersOffset + I3RC_CNT_PHOTONS]);
}

// The packed tally buffer of a grid: the fields of i3rc_tally_layout one behind the other, then the extra block, so that switching it
// moves no other offset.  Fills L, and V's offsets and sizes (levelUp / levelDown: -1 unless the block is EXTRA_LEVELS; pathUp1 ...
// pathDown2: -1 unless it is EXTRA_PATHS; radiancePath1 / radiancePath2: -1 unless it is EXTRA_RADIANCE_PATHS); returns the extra block's
// offset, -1 without one.  (nBins: the path histogram's, see path_bin_block_words; its fields lie at path_bin_field from the offset
// returned -- the view has no words for them)
inline long long tally_layout(int nx, int ny, int nz, int ncomp, int nDir, ExtraTally extra, i3rc_tally_layout &L, TallyView &V, int nBins = 0) {
  const long long ncol = (long long)nx * ny;
  long long o = 0;
  L.fluxUp = o; o += ncol;
  L.fluxDown = o; o += ncol;
  L.fluxAbsorbed = o; o += ncol;
  L.volumeAbsorption = o; o += ncol * nz;
  L.intensityByComponent = o; o += (long long)(ncomp + 1) * nDir * ncol;
  L.intensityExcess = o; o += (long long)(ncomp + 1) * nDir;
  L.counters = o; o += I3RC_NUM_COUNTERS;
  const long long block = extra == EXTRA_NONE ? -1 : extra_block_offset(L.counters);
  L.total = o + (extra == EXTRA_PATH_BINS        ? path_bin_block_words(nBins)
                 : extra == EXTRA_RADIANCE_PATHS ? radiance_path_block_words(nDir, nx, ny)
                                                 : extra_block_words(extra, nx, ny, nz));
  V.fluxUp = L.fluxUp; V.fluxDown = L.fluxDown; V.fluxAbsorbed = L.fluxAbsorbed; V.volumeAbsorption = L.volumeAbsorption;
  V.intensityByComponent = L.intensityByComponent; V.intensityExcess = L.intensityExcess; V.counters = L.counters;
  V.levelUp = extra == EXTRA_LEVELS ? block : -1;
  V.levelDown = extra == EXTRA_LEVELS ? block + (nz + 1) * ncol : -1;
  V.pathUp1 = extra == EXTRA_PATHS ? block : -1;
  V.pathUp2 = extra == EXTRA_PATHS ? block + ncol : -1;
  V.pathDown1 = extra == EXTRA_PATHS ? block + 2 * ncol : -1;
  V.pathDown2 = extra == EXTRA_PATHS ? block + 3 * ncol : -1;
  V.radiancePath1 = extra == EXTRA_RADIANCE_PATHS ? block : -1;
  V.radiancePath2 = extra == EXTRA_RADIANCE_PATHS ? block + (long long)nDir * ncol : -1;
  V.nx = nx; V.ny = ny; V.nz = nz; V.ncomp = ncomp; V.nDir = nDir;
  return block;
}

// What the rule needs of the grid, from its float32 edges: every column's share of the domain's area and every layer's depth.
inline void grid_fractions(int nx, int ny, int nz, const float *xE, const float *yE, const float *zE, double *areaFrac, double *dz) {
  for (int k = 0; k < nz; ++k) dz[k] = (double)zE[k + 1] - zE[k];
  const double ax = (double)xE[nx] - xE[0], ay = (double)yE[ny] - yE[0];
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) areaFrac[(long long)j * nx + i] = (((double)yE[j + 1] - yE[j]) * ((double)xE[i + 1] - xE[i])) / (ax * ay);
}

// photons per column :353-367 (float64 here; the reference works in real(4))
I3RC_TALLY_FN double photons_per_column(const TallyView &V, const double *raw, long long col) {
  const double nPhot = raw[V.counters + I3RC_CNT_PHOTONS];
  return V.xyRegular ? nPhot / (double)(V.nx * V.ny) : V.areaFrac[col] * nPhot;
}

// fluxUp, fluxDown, fluxAbsorbed and the level fluxes (:368-376): `at` is the element's offset in the block, `col` its column
I3RC_TALLY_FN float normalised_column_flux(const TallyView &V, const double *raw, long long at, long long col) {
  return (float)(raw[at] / photons_per_column(V, raw, col));
}

I3RC_TALLY_FN float normalised_volume_absorption(const TallyView &V, const double *raw, int kz, long long col) {
  const long long ncol = (long long)V.nx * V.ny;
  return (float)(raw[V.volumeAbsorption + kz * ncol + col] / (photons_per_column(V, raw, col) * V.dz[kz]));
}

// The cell-mean actinic flux from the track-length sums (the EXTRA_TRACKS block at `block`, [nz][ny][nx]):
// per photon of the column and per unit of the layer's depth, as volumeAbsorption -- 1 in clear air under a zenith sun, in units of the
// incident flux on a horizontal surface.
I3RC_TALLY_FN float normalised_actinic_flux(const TallyView &V, const double *raw, long long block, int kz, long long col) {
  const long long ncol = (long long)V.nx * V.ny;
  return (float)(raw[block + kz * ncol + col] / (photons_per_column(V, raw, col) * V.dz[kz]));
}

// Element e of the kind's extra block (at `block`) as reportResults hands it out: the level fluxes (e counts through levelFluxUp |
// levelFluxDown, level after level) and the path-length sums (e counts through pathUp1 | pathUp2 | pathDown1 | pathDown2) per photon of
// the column, as fluxUp; the actinic flux also per unit of the layer's depth; the radiance path sums (e counts through radiancePath1 |
// radiancePath2, direction after direction) per photon of the column, as the radiance word they belong to (normalised_intensity without
// an excess: the kind is refused with the contribution limit).  What i3rc_hip_normalise_level_fluxes / _actinic_flux / _path_lengths /
// _radiance_path_lengths fill their arrays with and what the diagnostic batch moments add up.
I3RC_TALLY_FN float normalised_extra_value(const TallyView &V, const double *raw, ExtraTally kind, long long block, long long e) {
  const long long ncol = (long long)V.nx * V.ny;
  if (kind == EXTRA_TRACKS) {
    const int kz = (int)(e / ncol);
    return normalised_actinic_flux(V, raw, block, kz, e - kz * ncol);
  }
  // (the path histogram: e counts through binUp | binPathUp | binDown | binPathDown, per photon of the block and not per column)
  if (kind == EXTRA_PATH_BINS) return normalised_path_bin(raw, V.counters, block + e);
  return normalised_column_flux(V, raw, block + e, e % ncol);
}

// THE DIAGNOSTIC BATCH MOMENTS (i3rc_hip_run_batches_diagnostic_moments): where the sums over a loop's batches of the kind's fields and
// of their domain means -- float32(sum over the columns / number of columns) per level or layer, a plain column mean on every grid --
// lie in a block of their own, in float64 words.  EXTRA_NONE: total 0.
struct ExtraMomentsLayout {
  long long levelFluxUp, levelFluxDown, meanLevelFluxUp, meanLevelFluxDown;   // EXTRA_LEVELS: [nz + 1][ny][nx] twice, then nz + 1 twice
  long long actinicFlux, meanActinicFlux;                                    // EXTRA_TRACKS: [nz][ny][nx], then nz
  long long total;                                                           // (what the kind has not: -1)
};
I3RC_TALLY_FN ExtraMomentsLayout extra_moments_layout(ExtraTally kind, int nx, int ny, int nz) {
  const long long ncol = (long long)nx * ny;
  ExtraMomentsLayout L = {-1, -1, -1, -1, -1, -1, 0};
  if (kind == EXTRA_LEVELS) {
    L.levelFluxUp = 0; L.levelFluxDown = (nz + 1) * ncol;
    L.meanLevelFluxUp = 2 * (nz + 1) * ncol; L.meanLevelFluxDown = L.meanLevelFluxUp + (nz + 1);
    L.total = L.meanLevelFluxDown + (nz + 1);
  } else if (kind == EXTRA_TRACKS) {
    L.actinicFlux = 0; L.meanActinicFlux = ncol * nz;
    L.total = L.meanActinicFlux + nz;
  }
  return L;
}
// ... the fields in front of the means (= extra_block_words: the moments' fields lie as the block's elements do), and the means
I3RC_TALLY_FN long long extra_moments_means(ExtraTally kind, int nz) { return kind == EXTRA_LEVELS ? 2 * (nz + 1) : (kind == EXTRA_TRACKS ? nz : 0); }

// THE PATH MOMENTS (i3rc_hip_run_batches_path_moments): where the sums over a loop's batches of the two path tallies' results lie in a
// block of their own, in float64 words; what the kind has not is -1, and total is 0 for any other kind.
//   EXTRA_PATHS      the four fields [ny][nx] in the block's order, their plain column means (float32(sum over the columns / number of
//                    columns), as every other mean), then the DOMAIN's path figures: float32(sum over the columns of raw pathUp1 / sum
//                    over the columns of raw fluxUp) = <L> of the reflected light, the same of pathUp2 = <L^2>, and the two of the
//                    transmitted light over fluxDown; 0 where the denominator is 0.  The ratio of raw sums is the area-weighted one on every grid.
//   EXTRA_PATH_BINS  the four fields of nBins + 1 words, then for each of nK absorption coefficients the lower and the upper bound of
//                    sum_b u_b <exp(-k L)>_b / photons, of the reflected and of the transmitted light (path_spectrum_term below)
struct PathMomentsLayout {
  long long pathLengthUp, pathLengthSquaredUp, pathLengthDown, pathLengthSquaredDown;                   // [ny][nx] each
  long long meanPathLengthUp, meanPathLengthSquaredUp, meanPathLengthDown, meanPathLengthSquaredDown;   // 1 each
  long long domainPathUp, domainPathSquaredUp, domainPathDown, domainPathSquaredDown;                   // 1 each
  long long histogramUp, histogramPathUp, histogramDown, histogramPathDown;                             // nBins + 1 each
  long long spectrumUpLower, spectrumUpUpper, spectrumDownLower, spectrumDownUpper;                     // nK each
  long long total;
};
constexpr int kPathMomentsWords = 21;   // (the words of PathMomentsLayout, in order: i3rc_hip_path_moments_layout_words)
constexpr int kMaxPathSpectrum = 256;   // (i3rc_hip_set_path_spectrum: 0 <= nK <= 256)
I3RC_TALLY_FN PathMomentsLayout path_moments_layout(ExtraTally kind, int nx, int ny, int nBins, int nK) {
  const long long ncol = (long long)nx * ny, nb = (long long)nBins + 1;
  PathMomentsLayout L = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
  if (kind == EXTRA_PATHS) {
    L.pathLengthUp = 0; L.pathLengthSquaredUp = ncol; L.pathLengthDown = 2 * ncol; L.pathLengthSquaredDown = 3 * ncol;
    L.meanPathLengthUp = 4 * ncol; L.meanPathLengthSquaredUp = 4 * ncol + 1; L.meanPathLengthDown = 4 * ncol + 2; L.meanPathLengthSquaredDown = 4 * ncol + 3;
    L.domainPathUp = 4 * ncol + 4; L.domainPathSquaredUp = 4 * ncol + 5; L.domainPathDown = 4 * ncol + 6; L.domainPathSquaredDown = 4 * ncol + 7;
    L.total = 4 * ncol + 8;
  } else if (kind == EXTRA_PATH_BINS) {
    L.histogramUp = 0; L.histogramPathUp = nb; L.histogramDown = 2 * nb; L.histogramPathDown = 3 * nb;
    L.spectrumUpLower = 4 * nb; L.spectrumUpUpper = 4 * nb + nK; L.spectrumDownLower = 4 * nb + 2 * (long long)nK; L.spectrumDownUpper = 4 * nb + 3 * (long long)nK;
    L.total = 4 * nb + 4 * (long long)nK;
  }
  return L;
}
// ... the fields in front of the other quantities (they lie as the block's elements do), and the number of those quantities
I3RC_TALLY_FN long long path_moments_fields(ExtraTally kind, int nx, int ny, int nBins) {
  return kind == EXTRA_PATHS ? 4 * (long long)nx * ny : (kind == EXTRA_PATH_BINS ? path_bin_block_words(nBins) : 0);
}
I3RC_TALLY_FN int path_moments_quantities(ExtraTally kind, int nK) { return kind == EXTRA_PATHS ? 8 : (kind == EXTRA_PATH_BINS ? 4 * nK : 0); }

// What bin b (nBins: the overflow bin) of raw weight u and raw path sum p adds to the two bounds of sum_b u_b <exp(-k L)>_b, in
// float64: the bin's mean path m = p / u, clamped to the bin's float32 edges, gives u exp(-k m) from below (Jensen) and the chord over
// the bin from above; the overflow bin has no upper edge, so its mean path is only kept above its edge and its upper bound is
// u exp(-k edge).  An empty bin adds nothing.  Edges: as path_bin's.
template <class Edges>
I3RC_TALLY_FN void path_spectrum_term(Edges edges, int nBins, int b, double u, double p, double k, double &lower, double &upper) {
  lower = 0.0; upper = 0.0;
  if (!(u > 0.0)) return;
  const double e0 = (double)edges[b < nBins ? b : nBins];
  double m = p / u;
  m = m < e0 ? e0 : m;
  if (b >= nBins) {
    lower = u * ::exp(-k * m);
    upper = u * ::exp(-k * e0);
    return;
  }
  const double e1 = (double)edges[b + 1];
  m = m > e1 ? e1 : m;
  lower = u * ::exp(-k * m);
  upper = u * ((e1 - m) * ::exp(-k * e0) + (m - e0) * ::exp(-k * e1)) / (e1 - e0);
}
// ... and a domain path figure from the two raw sums over the columns
I3RC_TALLY_FN float domain_path_ratio(double pathSum, double fluxSum) { return fluxSum > 0.0 ? (float)(pathSum / fluxSum) : 0.0f; }

// What component j (0: the surface) adds to the column's radiance in direction d beyond its own sum: its share of the excess of
// limited contributions, in proportion to the field (:327-347).  excessSums[j * nDir + d] = the sum over the columns of component j's
// field in direction d; the caller forms it (the host sequentially, moments_excess_kernel in a tree).
I3RC_TALLY_FN double excess_share(const TallyView &V, const double *raw, const double *excessSums, int j, int d, double own) {
  const double ex = raw[V.intensityExcess + (long long)j * V.nDir + d];
  return (own / excessSums[j * V.nDir + d]) * ex;
}
I3RC_TALLY_FN bool has_excess(const TallyView &V, const double *raw, int j, int d) {
  return V.limitContrib && raw[V.intensityExcess + (long long)j * V.nDir + d] > 0.0;
}

// intensity = the sum over the components of intensityByComponent (:574-579, :662-667), then the excess, then per photon of the column
I3RC_TALLY_FN float normalised_intensity(const TallyView &V, const double *raw, const double *excessSums, int d, long long col) {
  const long long ncol = (long long)V.nx * V.ny;
  const double *f = raw + V.intensityByComponent + d * ncol + col;
  double tot = 0.0;
  for (int j = 0; j <= V.ncomp; ++j) tot += f[(long long)j * V.nDir * ncol];
  for (int j = 0; j <= V.ncomp; ++j)
    if (has_excess(V, raw, j, d)) tot += excess_share(V, raw, excessSums, j, d, f[(long long)j * V.nDir * ncol]);
  return (float)(tot / photons_per_column(V, raw, col));
}

// (the reference leaves component 0 un-normalised: :390 loops j = 1:numComponents)
I3RC_TALLY_FN float normalised_intensity_by_component(const TallyView &V, const double *raw, const double *excessSums, int j, int d, long long col) {
  const long long ncol = (long long)V.nx * V.ny;
  double v = raw[V.intensityByComponent + ((long long)j * V.nDir + d) * ncol + col];
  if (has_excess(V, raw, j, d)) v += excess_share(V, raw, excessSums, j, d, v);
  return (float)(j == 0 ? v : v / photons_per_column(V, raw, col));
}

}  // namespace i3rc
