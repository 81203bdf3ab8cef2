// Stand-alone driver of csrc/tally_block.hpp for tests/test_radiance_path_lengths_cpu.py: host C++17, no HIP.
//   radiance_path_main IN OUT
// IN:  6 int64 -- nx, ny, nz, xyRegular, ncomp, nDir --, the float32 edges x[nx + 1], y[ny + 1], z[nz + 1], the raw float64 block of a
//      radiance problem with the radiance path block, as long as the header's layout (tally_layout) says.
// OUT: 50 int64 -- with the kind on: the view's two offsets, the extra block's offset, the counters' offset and the block's total; then for
//      each other kind (none, levels, tracks, paths, the path histogram of 7 bins) the view's two radiance path offsets, its two level
//      offsets, its four path offsets and its total, all from the header --, then float32 intensity [nDir][ny][nx]
//      (normalised_intensity, no contribution limit) and radiancePathLength | radiancePathLengthSquared (normalised_extra_value, element
//      after element of the block).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(6);
  if (!in || !read(in, s)) return 3;
  const int ncomp = (int)s[4], nDir = (int)s[5];
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout((int)s[0], (int)s[1], (int)s[2], ncomp, nDir, i3rc::EXTRA_RADIANCE_PATHS, lay, V);
  V.xyRegular = (int)s[3]; V.limitContrib = 0;
  const size_t ncol = (size_t)V.nx * V.ny;
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1);
  std::vector<double> raw((size_t)lay.total), areaFrac(ncol), dz((size_t)V.nz);
  if (!read(in, xE) || !read(in, yE) || !read(in, zE) || !read(in, raw)) return 3;
  std::fclose(in);
  i3rc::grid_fractions(V.nx, V.ny, V.nz, xE.data(), yE.data(), zE.data(), areaFrac.data(), dz.data());
  V.areaFrac = areaFrac.data(); V.dz = dz.data();

  std::vector<float> out;
  for (int d = 0; d < nDir; ++d)
    for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_intensity(V, raw.data(), nullptr, d, (long long)k));
  const long long words = i3rc::radiance_path_block_words(nDir, V.nx, V.ny);
  for (long long e = 0; e < words; ++e) out.push_back(i3rc::normalised_extra_value(V, raw.data(), i3rc::EXTRA_RADIANCE_PATHS, block, e));

  std::vector<int64_t> offsets = {V.radiancePath1, V.radiancePath2, block, V.counters, lay.total};
  for (const i3rc::ExtraTally other : {i3rc::EXTRA_NONE, i3rc::EXTRA_LEVELS, i3rc::EXTRA_TRACKS, i3rc::EXTRA_PATHS, i3rc::EXTRA_PATH_BINS}) {
    i3rc_tally_layout l2{};
    i3rc::TallyView v2{};
    (void)i3rc::tally_layout(V.nx, V.ny, V.nz, ncomp, nDir, other, l2, v2, other == i3rc::EXTRA_PATH_BINS ? 7 : 0);
    for (const long long w : {v2.radiancePath1, v2.radiancePath2, v2.levelUp, v2.levelDown, v2.pathUp1, v2.pathUp2, v2.pathDown1, v2.pathDown2, (long long)l2.total})
      offsets.push_back(w);
  }
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(offsets.data(), sizeof(int64_t), offsets.size(), o) != offsets.size() || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) return 4;
  return 0;
}
