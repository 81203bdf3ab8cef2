// Stand-alone driver of csrc/pass_decision.hpp for tests/test_pass_decision_cpu.py: host C++17, no HIP.
//   pass_decision_main IN OUT
//     IN:  records of five int32 -- nSc, nTu, trEmpty (0 / 1), evThr, quorums (0: kTurnMin 4, kTurnForce 12; 1: both 1) --, as many as
//          the file holds.
//     OUT: per record one int32: pass_decision<kTurnMin, kTurnForce>(nSc, nTu, trEmpty != 0, evThr), the bits of i3rc::PassBits.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pass_decision.hpp"

static_assert(i3rc::kPassStop == 1 && i3rc::kPassEvent == 2 && i3rc::kPassTurn == 4, "the test reads the bits by these values");

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
  if (!in || !o) return 3;
  std::vector<int32_t> out;
  int32_t rec[5];
  while (std::fread(rec, sizeof(int32_t), 5, in) == 5) {
    if (rec[4] != 0 && rec[4] != 1) return 5;
    out.push_back(rec[4] == 0 ? i3rc::pass_decision<4, 12>(rec[0], rec[1], rec[2] != 0, rec[3])
                              : i3rc::pass_decision<1, 1>(rec[0], rec[1], rec[2] != 0, rec[3]));
  }
  std::fclose(in);
  const bool ok = std::fwrite(out.data(), sizeof(int32_t), out.size(), o) == out.size();
  return std::fclose(o) != 0 || !ok ? 4 : 0;
}
