// Stand-alone driver of csrc/event_flags.hpp for tests/test_event_flags_roulette_cpu.py: host C++17, no HIP.
//   event_flags_roulette_main IN OUT
//     IN:  records of five 32-bit words -- float32 uniformSsa, int32 uniformPf, int32 brdfGrid, float32 albedo, int32 useRoulette --, as
//          many as the file holds.
//     OUT: in front, four uint32: kWeightStaysOne, kNoAbsorption, kNeedCell, kPlaysRoulette; then two uint32 per record: event_flags called
//          with four arguments (as the callers from before the roulette bit call it) and with all five.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "event_flags.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
  if (!in || !o) return 3;
  std::vector<uint32_t> out = {i3rc::kWeightStaysOne, i3rc::kNoAbsorption, i3rc::kNeedCell, i3rc::kPlaysRoulette};
  uint32_t rec[5];
  while (std::fread(rec, sizeof(uint32_t), 5, in) == 5) {
    float ssa, albedo;
    int32_t pf, brdf, roulette;
    std::memcpy(&ssa, &rec[0], 4); std::memcpy(&pf, &rec[1], 4); std::memcpy(&brdf, &rec[2], 4); std::memcpy(&albedo, &rec[3], 4);
    std::memcpy(&roulette, &rec[4], 4);
    out.push_back(i3rc::event_flags(ssa, pf, brdf != 0, albedo));
    out.push_back(i3rc::event_flags(ssa, pf, brdf != 0, albedo, roulette != 0));
  }
  std::fclose(in);
  const bool ok = std::fwrite(out.data(), sizeof(uint32_t), out.size(), o) == out.size();
  return std::fclose(o) != 0 || !ok ? 4 : 0;
}
