// Stand-alone driver of csrc/tally_block.hpp for tests/test_path_histogram_cpu.py: host C++17, no HIP.
//   path_histogram_main layout IN OUT
//     IN:  4 int64 -- nx, ny, nz, nBins --, then the raw float64 block of a flux problem (one component, no directions) with the
//          histogram's block, as long as the header's layout (tally_layout) says.
//     OUT: 33 int64 -- the four fields' offsets (block + path_bin_field), the block's offset, its length (path_bin_block_words), the
//          counters' offset and the total; then for each other kind (none, levels, tracks, paths) its four path offsets and its total,
//          all from the header; the view's four path offsets and level offset of the histogram's own view --, then float32
//          binUp | binPathUp | binDown | binPathDown (normalised_path_bin, word after word of the block).
//   path_histogram_main bins IN OUT
//     IN:  2 int64 -- nBins, the number of values --, the nBins + 1 float32 edges, the float32 values.
//     OUT: one int32 per value: path_bin.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tally_block.hpp"

template <class T>
static bool read(std::FILE *f, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T>
static bool write(std::FILE *f, const std::vector<T> &v) { return std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int layout(std::FILE *in, std::FILE *o) {
  std::vector<int64_t> s(4);
  if (!read(in, s)) return 3;
  const int nx = (int)s[0], ny = (int)s[1], nz = (int)s[2], nBins = (int)s[3];
  i3rc_tally_layout lay{};
  i3rc::TallyView V{};
  const long long block = i3rc::tally_layout(nx, ny, nz, 1, 0, i3rc::EXTRA_PATH_BINS, lay, V, nBins);
  std::vector<double> raw((size_t)lay.total);
  if (!read(in, raw)) return 3;
  const long long words = i3rc::path_bin_block_words(nBins);
  std::vector<float> out;
  for (long long e = 0; e < words; ++e) out.push_back(i3rc::normalised_path_bin(raw.data(), V.counters, block + e));
  std::vector<int64_t> offsets;
  for (int f = 0; f < 4; ++f) offsets.push_back(block + i3rc::path_bin_field(f, nBins));
  for (const long long w : {block, words, V.counters, (long long)lay.total}) offsets.push_back(w);
  for (const i3rc::ExtraTally other : {i3rc::EXTRA_NONE, i3rc::EXTRA_LEVELS, i3rc::EXTRA_TRACKS, i3rc::EXTRA_PATHS}) {
    i3rc_tally_layout l2{};
    i3rc::TallyView v2{};
    (void)i3rc::tally_layout(nx, ny, nz, 1, 0, other, l2, v2);
    for (const long long w : {v2.pathUp1, v2.pathUp2, v2.pathDown1, v2.pathDown2, (long long)l2.total}) offsets.push_back(w);
  }
  for (const long long w : {V.pathUp1, V.pathUp2, V.pathDown1, V.pathDown2, V.levelUp}) offsets.push_back(w);
  return write(o, offsets) && write(o, out) ? 0 : 4;
}

static int bins(std::FILE *in, std::FILE *o) {
  std::vector<int64_t> s(2);
  if (!read(in, s)) return 3;
  const int nBins = (int)s[0];
  std::vector<float> edges((size_t)nBins + 1), x((size_t)s[1]);
  if (!read(in, edges) || !read(in, x)) return 3;
  std::vector<int32_t> out;
  for (const float v : x) out.push_back(i3rc::path_bin(edges.data(), nBins, v));
  return write(o, out) ? 0 : 4;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  std::FILE *in = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
  if (!in || !o) return 3;
  const int rc = std::strcmp(argv[1], "layout") == 0 ? layout(in, o) : std::strcmp(argv[1], "bins") == 0 ? bins(in, o) : 2;
  std::fclose(in);
  return std::fclose(o) != 0 && rc == 0 ? 4 : rc;
}
