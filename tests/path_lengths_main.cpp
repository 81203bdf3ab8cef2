// Stand-alone driver of csrc/tally_block.hpp for tests/test_path_lengths_cpu.py: host C++17, no HIP.
//   path_lengths_main IN OUT
// IN:  4 int64 -- nx, ny, nz, xyRegular --, the float32 edges x[nx + 1], y[ny + 1], z[nz + 1], the raw float64 block of a flux problem
//      (one component, no directions) with the path-length block, as long as the header's layout (tally_layout) says.
// OUT: 25 int64 -- the view's four path offsets, the extra block's offset, its length (extra_block_words), the counters' offset and the
//      block's total; the view's two level offsets; and for each other kind (none, levels, tracks) its four path offsets and its total,
//      all from the header --, then float32 fluxUp | fluxDown (normalised_column_flux) and pathLengthUp |
//      pathLengthSquaredUp | pathLengthDown | pathLengthSquaredDown (normalised_extra_value, element after element of the block).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  std::vector<int64_t> s(4);
  if (!in || !read(in, s)) return 3;
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout((int)s[0], (int)s[1], (int)s[2], 1, 0, i3rc::EXTRA_PATHS, lay, V);
  V.xyRegular = (int)s[3]; V.limitContrib = 0;
  const size_t ncol = (size_t)V.nx * V.ny;
  std::vector<float> xE(V.nx + 1), yE(V.ny + 1), zE(V.nz + 1);
  std::vector<double> raw((size_t)lay.total), areaFrac(ncol), dz((size_t)V.nz);
  if (!read(in, xE) || !read(in, yE) || !read(in, zE) || !read(in, raw)) return 3;
  std::fclose(in);
  i3rc::grid_fractions(V.nx, V.ny, V.nz, xE.data(), yE.data(), zE.data(), areaFrac.data(), dz.data());
  V.areaFrac = areaFrac.data(); V.dz = dz.data();

  std::vector<float> out;
  for (const long long at : {V.fluxUp, V.fluxDown})
    for (size_t k = 0; k < ncol; ++k) out.push_back(i3rc::normalised_column_flux(V, raw.data(), at + (long long)k, (long long)k));
  const long long words = i3rc::extra_block_words(i3rc::EXTRA_PATHS, V.nx, V.ny, V.nz);
  for (long long e = 0; e < words; ++e) out.push_back(i3rc::normalised_extra_value(V, raw.data(), i3rc::EXTRA_PATHS, block, e));

  std::vector<int64_t> offsets = {V.pathUp1, V.pathUp2, V.pathDown1, V.pathDown2, block, words, V.counters, lay.total, V.levelUp, V.levelDown};
  for (const i3rc::ExtraTally other : {i3rc::EXTRA_NONE, i3rc::EXTRA_LEVELS, i3rc::EXTRA_TRACKS}) {
    i3rc_tally_layout l2{};
    i3rc::TallyView v2{};
    (void)i3rc::tally_layout(V.nx, V.ny, V.nz, 1, 0, other, l2, v2);
    for (const long long w : {v2.pathUp1, v2.pathUp2, v2.pathDown1, v2.pathDown2, (long long)l2.total}) offsets.push_back(w);
  }
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(offsets.data(), sizeof(int64_t), offsets.size(), o) != offsets.size() || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) return 4;
  return 0;
}
