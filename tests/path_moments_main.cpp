// Stand-alone driver of csrc/tally_block.hpp for tests/test_path_moments_cpu.py: host C++17, no HIP.
//   path_moments_main IN OUT
// IN:  7 int64 -- nx, ny, nz, xyRegular, the kind of the extra block (ExtraTally: 3 path lengths, 4 the path histogram), nBins, nK --,
//      the float32 edges x[nx + 1], y[ny + 1], z[nz + 1], for the histogram its float32 edges[nBins + 1] and absorption[nK], then the
//      raw float64 block, as long as the header's layout (tally_layout, one component, no directions) says.
// OUT: 22 int64 -- the extra block's offset and the words of path_moments_layout --, then one float32 per word of that layout: what a
//      batch adds to the path moments -- the fields (normalised_extra_value), the column means and the domain's path figures
//      (domain_path_ratio), or the spectrum's bounds (path_spectrum_term) --, every sum taken in the order of its elements.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(7);
  if (!in || !read(in, s) || (s[4] != i3rc::EXTRA_PATHS && s[4] != i3rc::EXTRA_PATH_BINS)) return 3;
  const i3rc::ExtraTally kind = (i3rc::ExtraTally)s[4];
  const int nBins = (int)s[5], nK = (int)s[6];
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout((int)s[0], (int)s[1], (int)s[2], 1, 0, kind, lay, V, nBins);
  V.xyRegular = (int)s[3];
  const long long ncol = (long long)V.nx * V.ny;
  const bool bins = kind == i3rc::EXTRA_PATH_BINS;
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1), edges(bins ? nBins + 1 : 0), absorption(bins ? nK : 0);
  std::vector<double> raw((size_t)lay.total), areaFrac((size_t)ncol), dz((size_t)V.nz);
  if (!read(in, xE) || !read(in, yE) || !read(in, zE) || !read(in, edges) || !read(in, absorption) || !read(in, raw)) return 3;
  std::fclose(in);
  i3rc::grid_fractions(V.nx, V.ny, V.nz, xE.data(), yE.data(), zE.data(), areaFrac.data(), dz.data());
  V.areaFrac = areaFrac.data(); V.dz = dz.data();

  const i3rc::PathMomentsLayout L = i3rc::path_moments_layout(kind, V.nx, V.ny, nBins, nK);
  const long long fields = i3rc::path_moments_fields(kind, V.nx, V.ny, nBins);
  std::vector<float> out;
  for (long long e = 0; e < fields; ++e) out.push_back(i3rc::normalised_extra_value(V, raw.data(), kind, block, e));
  if (!bins) {
    for (int f = 0; f < 4; ++f) {   // the plain column means
      double v = 0.0;
      for (long long k = 0; k < ncol; ++k) v += (double)out[(size_t)(f * ncol + k)];
      out.push_back((float)(v / (double)ncol));
    }
    for (int f = 0; f < 4; ++f) {   // the domain's <L>, <L^2>: reflected over fluxUp, transmitted over fluxDown
      double num = 0.0, den = 0.0;
      for (long long k = 0; k < ncol; ++k) { num += raw[(size_t)(block + f * ncol + k)]; den += raw[(size_t)((f < 2 ? V.fluxUp : V.fluxDown) + k)]; }
      out.push_back(i3rc::domain_path_ratio(num, den));
    }
  } else {
    for (int which = 0; which < 4; ++which)   // spectrumUpLower | UpUpper | DownLower | DownUpper
      for (int j = 0; j < nK; ++j) {
        const double *weight = raw.data() + block + i3rc::path_bin_field(which < 2 ? 0 : 2, nBins), *path = weight + (nBins + 1);
        double v = 0.0;
        for (int b = 0; b <= nBins; ++b) {
          double lower, upper;
          i3rc::path_spectrum_term(edges.data(), nBins, b, weight[b], path[b], (double)absorption[(size_t)j], lower, upper);
          v += (which & 1) ? upper : lower;
        }
        out.push_back((float)(v / raw[(size_t)(V.counters + I3RC_CNT_PHOTONS)]));
      }
  }
  if ((long long)out.size() != L.total) return 5;

  const int64_t header[1 + i3rc::kPathMomentsWords] = {
      block, L.pathLengthUp, L.pathLengthSquaredUp, L.pathLengthDown, L.pathLengthSquaredDown, L.meanPathLengthUp, L.meanPathLengthSquaredUp,
      L.meanPathLengthDown, L.meanPathLengthSquaredDown, L.domainPathUp, L.domainPathSquaredUp, L.domainPathDown, L.domainPathSquaredDown,
      L.histogramUp, L.histogramPathUp, L.histogramDown, L.histogramPathDown, L.spectrumUpLower, L.spectrumUpUpper, L.spectrumDownLower,
      L.spectrumDownUpper, L.total};
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(header, sizeof(int64_t), 1 + i3rc::kPathMomentsWords, o) != 1 + i3rc::kPathMomentsWords ||
      std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0)
    return 4;
  return 0;
}
