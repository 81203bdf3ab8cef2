// Stand-alone driver of csrc/tally_block.hpp for tests/test_normalise_cpu.py: host C++17, no HIP.
//   normalise_main IN OUT
// IN:  8 int64 -- nx, ny, nz, ncomp, nDir, xyRegular, limitContrib and the kind of the extra block (ExtraTally) --, the float32 edges
//      x[nx + 1], y[ny + 1], z[nz + 1], the raw float64 block, as long as the header's layout (tally_layout) says.
// OUT: 11 int64 -- the view's nine offsets (fluxUp ... levelDown), the extra block's offset and the block's length, all from the header --,
//      then float32 fluxUp | fluxDown | fluxAbsorbed | volumeAbsorption | intensity | intensityByComponent, and levelFluxUp | levelFluxDown
//      (EXTRA_LEVELS) or actinicFlux (EXTRA_TRACKS).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(8);
  if (!in || !read(in, s) || s[7] < i3rc::EXTRA_NONE || s[7] > i3rc::EXTRA_TRACKS) return 3;
  const i3rc::ExtraTally extra = (i3rc::ExtraTally)s[7];
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout((int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4], extra, lay, V);
  V.xyRegular = (int)s[5]; V.limitContrib = (int)s[6];
  const size_t ncol = (size_t)V.nx * V.ny;
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1);
  std::vector<double> raw((size_t)lay.total), areaFrac(ncol), dz((size_t)V.nz);
  if (!read(in, xE) || !read(in, yE) || !read(in, zE) || !read(in, raw)) return 3;
  std::fclose(in);
  i3rc::grid_fractions(V.nx, V.ny, V.nz, xE.data(), yE.data(), zE.data(), areaFrac.data(), dz.data());
  V.areaFrac = areaFrac.data(); V.dz = dz.data();

  std::vector<float> out;
  for (const long long at : {V.fluxUp, V.fluxDown, V.fluxAbsorbed})
    for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_column_flux(V, raw.data(), at + (long long)k, (long long)k));
  for (int kz = 0; kz < V.nz; ++kz)
    for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_volume_absorption(V, raw.data(), kz, (long long)k));
  std::vector<double> excessSums((size_t)(V.ncomp + 1) * V.nDir, 0.0);   // column after column, as i3rc_hip_normalise adds them up
  for (size_t jd = 0; jd < excessSums.size(); ++jd)
    for (size_t k = 0; k < ncol; ++k) excessSums[jd] += raw[(size_t)V.intensityByComponent + jd * ncol + k];
  for (int d = 0; d < V.nDir; ++d)
    for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_intensity(V, raw.data(), excessSums.data(), d, (long long)k));
  for (int j = 0; j <= V.ncomp; ++j)
    for (int d = 0; d < V.nDir; ++d)
      for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_intensity_by_component(V, raw.data(), excessSums.data(), j, d, (long long)k));
  if (extra == i3rc::EXTRA_LEVELS)
    for (const long long at : {V.levelUp, V.levelDown})
      for (size_t e = 0; e < (size_t)(V.nz + 1) * ncol; ++e) out.push_back(i3rc::normalised_column_flux(V, raw.data(), at + (long long)e, (long long)(e % ncol)));
  if (extra == i3rc::EXTRA_TRACKS)
    for (int kz = 0; kz < V.nz; ++kz)
      for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_actinic_flux(V, raw.data(), block, kz, (long long)k));

  const int64_t offsets[11] = {V.fluxUp, V.fluxDown, V.fluxAbsorbed, V.volumeAbsorption, V.intensityByComponent, V.intensityExcess, V.counters,
                               V.levelUp, V.levelDown, block, lay.total};
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(offsets, sizeof(int64_t), 11, o) != 11 || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) return 4;
  return 0;
}
