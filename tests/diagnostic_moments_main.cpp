// Stand-alone driver of csrc/tally_block.hpp for tests/test_diagnostic_moments_cpu.py: host C++17, no HIP.
//   diagnostic_moments_main IN OUT
// IN:  5 int64 -- nx, ny, nz, xyRegular and the kind of the extra block (ExtraTally: 1 or 2) --, the float32 edges x[nx + 1], y[ny + 1],
//      z[nz + 1], the raw float64 block, as long as the header's layout (tally_layout, one component, no directions) says.
// OUT: 9 int64 -- the extra block's offset, the number of its elements, and the seven words of extra_moments_layout --, then float32
//      normalised_extra_value of every element of the block, then the same elements from normalised_column_flux /
//      normalised_actinic_flux evaluated directly.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(5);
  if (!in || !read(in, s) || s[4] < i3rc::EXTRA_LEVELS || s[4] > i3rc::EXTRA_TRACKS) return 3;
  const i3rc::ExtraTally kind = (i3rc::ExtraTally)s[4];
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout((int)s[0], (int)s[1], (int)s[2], 1, 0, kind, lay, V);
  V.xyRegular = (int)s[3];
  const long long ncol = (long long)V.nx * V.ny, words = i3rc::extra_block_words(kind, V.nx, V.ny, V.nz);
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1);
  std::vector<double> raw((size_t)lay.total), areaFrac((size_t)ncol), dz((size_t)V.nz);
  if (!read(in, xE) || !read(in, yE) || !read(in, zE) || !read(in, raw)) return 3;
  std::fclose(in);
  i3rc::grid_fractions(V.nx, V.ny, V.nz, xE.data(), yE.data(), zE.data(), areaFrac.data(), dz.data());
  V.areaFrac = areaFrac.data(); V.dz = dz.data();

  std::vector<float> out;
  for (long long e = 0; e < words; ++e) out.push_back(i3rc::normalised_extra_value(V, raw.data(), kind, block, e));
  if (kind == i3rc::EXTRA_LEVELS) {
    for (const long long at : {V.levelUp, V.levelDown})
      for (long long e = 0; e < (V.nz + 1) * ncol; ++e) out.push_back(i3rc::normalised_column_flux(V, raw.data(), at + e, e % ncol));
  } else {
    for (int kz = 0; kz < V.nz; ++kz)
      for (long long k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_actinic_flux(V, raw.data(), block, kz, k));
  }

  const i3rc::ExtraMomentsLayout L = i3rc::extra_moments_layout(kind, V.nx, V.ny, V.nz);
  const int64_t header[9] = {block, words, L.levelFluxUp, L.levelFluxDown, L.meanLevelFluxUp, L.meanLevelFluxDown, L.actinicFlux, L.meanActinicFlux, L.total};
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(header, sizeof(int64_t), 9, o) != 9 || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) return 4;
  return 0;
}
