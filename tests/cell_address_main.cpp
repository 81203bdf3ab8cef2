// Stand-alone driver of csrc/cell_address.hpp for tests/test_cell_address_cpu.py: host C++17, no HIP.
//   cell_address_main IN OUT
//     IN:  records of six 32-bit words -- uint32 base, int32 nx, ny, ix, iy, iz (indices 1-based) --, as many as the file holds.
//     OUT: per record five uint32: cell_address_bias(base, nx, ny); cell_address(that bias, nx, ny, ix, iy, iz); cell_word(nx, ny, ix, iy, iz);
//          column_address_bias(base, nx, 3); column_address(that bias, nx, ix, iy, 3).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cell_address.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
  if (!in || !o) return 3;
  std::vector<uint32_t> out;
  uint32_t rec[6];
  while (std::fread(rec, sizeof(uint32_t), 6, in) == 6) {
    const uint32_t base = rec[0];
    const int nx = (int32_t)rec[1], ny = (int32_t)rec[2], ix = (int32_t)rec[3], iy = (int32_t)rec[4], iz = (int32_t)rec[5];
    const uint32_t bias = i3rc::cell_address_bias(base, nx, ny), colBias = i3rc::column_address_bias(base, nx, 3);
    out.push_back(bias);
    out.push_back(i3rc::cell_address(bias, nx, ny, ix, iy, iz));
    out.push_back(i3rc::cell_word(nx, ny, ix, iy, iz));
    out.push_back(colBias);
    out.push_back(i3rc::column_address(colBias, nx, ix, iy, 3));
  }
  std::fclose(in);
  const bool ok = std::fwrite(out.data(), sizeof(uint32_t), out.size(), o) == out.size();
  return std::fclose(o) != 0 || !ok ? 4 : 0;
}
