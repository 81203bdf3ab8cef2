// Stand-alone driver of csrc/event_flags.hpp for tests/test_event_flags_cpu.py: host C++17, no HIP.
//   event_flags_main IN OUT
//     IN:  records of four 32-bit words -- float32 uniformSsa, int32 uniformPf, int32 brdfGrid, float32 albedo --, as many as the file holds.
//     OUT: one uint32 per record: event_flags; in front of them three uint32: kWeightStaysOne, kNoAbsorption, kNeedCell.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "event_flags.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
  if (!in || !o) return 3;
  std::vector<uint32_t> out = {i3rc::kWeightStaysOne, i3rc::kNoAbsorption, i3rc::kNeedCell};
  uint32_t rec[4];
  while (std::fread(rec, sizeof(uint32_t), 4, in) == 4) {
    float ssa, albedo;
    int32_t pf, brdf;
    std::memcpy(&ssa, &rec[0], 4); std::memcpy(&pf, &rec[1], 4); std::memcpy(&brdf, &rec[2], 4); std::memcpy(&albedo, &rec[3], 4);
    out.push_back(i3rc::event_flags(ssa, pf, brdf != 0, albedo));
  }
  std::fclose(in);
  const bool ok = std::fwrite(out.data(), sizeof(uint32_t), out.size(), o) == out.size();
  return std::fclose(o) != 0 || !ok ? 4 : 0;
}
