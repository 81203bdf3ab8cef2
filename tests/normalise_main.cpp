// Stand-alone driver of csrc/tally_block.hpp for tests/test_normalise_cpu.py: host C++17, no HIP.
//   normalise_main IN OUT
// IN:  17 int64 -- the view's nine offsets (fluxUp ... levelDown), nx, ny, nz, ncomp, nDir, xyRegular, limitContrib, and the block's
//      length --, the float32 edges x[nx + 1], y[ny + 1], z[nz + 1], the raw float64 block.
// OUT: float32 fluxUp | fluxDown | fluxAbsorbed | volumeAbsorption | intensity | intensityByComponent | levelFluxUp | levelFluxDown
//      (the last two where the view has a level block).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(17);
  if (!in || !read(in, s)) return 3;
  i3rc::TallyView V{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], (int)s[9], (int)s[10], (int)s[11], (int)s[12], (int)s[13], (int)s[14], (int)s[15],
                    nullptr, nullptr};
  const size_t ncol = (size_t)V.nx * V.ny;
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1);
  std::vector<double> raw((size_t)s[16]), areaFrac(ncol), dz((size_t)V.nz);
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
  if (V.levelUp >= 0)
    for (const long long at : {V.levelUp, V.levelDown})
      for (size_t e = 0; e < (size_t)(V.nz + 1) * ncol; ++e) out.push_back(i3rc::normalised_column_flux(V, raw.data(), at + (long long)e, (long long)(e % ncol)));

  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) return 4;
  return 0;
}
